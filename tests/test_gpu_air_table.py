"""Cp_air from the AirTable in LDS (common.hpp: AirTable / air_table_eval,
lean_tile.hpp: air_table_issue / air_table_write) in the single-gas lean tile
kernels.

a. native.air_table_probe -- the kernels' block builder, LDS staging and
   evaluation, one workgroup -- against the host's table_eval, bit for bit, at
   every knot, its neighbours in double, both extrapolating ends, +-0, 1e300 and
   +inf, for tables of both modes; a NaN argument gives a NaN.
b. the tile kernels with the deck's Cp_air replaced -- by an 8-point table
   whose knots are quantiles of the run's own temperature field, so the lanes
   of one wave fall into every segment and both ends; by a 17-point table
   (evaluated with table_eval on the species pack) and by a 1-point one --
   against the plain per-cell CPU stepper, bit for bit after every call of the
   schedule, from a perturbed start (tests/perturb.py).

Every case asserts through DeviceSolver.lean_tile_last which geometry and which
table path ran."""
import functools
import math

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from tests.air_tables import TABLES, arguments, same_bits, segment
from tests.perturb import FIELDS, MIN_NX, SCHEDULE, perturb, sweep_deck
from tests.test_gpu_tile_shapes import BIG, SEED, _assert_equal, _cpu_reference, _gpu, _march
from tests.test_gpu_tile_staging import expected_stage

pytestmark = pytest.mark.gpu


# --- a. the evaluation alone --------------------------------------------------

@pytest.mark.parametrize("name", sorted(TABLES))
def test_device_table_eval_equals_host(gpu, name):
    nat = gpu.native()
    rows, mode = TABLES[name]
    x, y = [r[0] for r in rows], [r[1] for r in rows]
    xv = arguments(rows)
    assert len(xv) < 64
    got, m = nat.air_table_probe(x, y, xv + [math.nan])
    assert m == mode
    want = nat.table_eval(x, y, xv)
    assert same_bits(got[:-1], want), [(v, a, b) for v, a, b in zip(xv, got, want) if not same_bits([a], [b])]
    # (a one-point table is its value at every argument, table_eval's n == 1)
    assert math.isnan(got[-1]) if len(rows) > 1 else got[-1] == y[0]


# --- b. the tile kernels ------------------------------------------------------

# (threads per workgroup, cells per thread, tile height override, tile height)
GEOMS = [(64, 1, 16, 16), (128, 1, 8, 8), (256, 2, 0, 32)]
KINDS = {"quantile8": 1, "n17": 0, "n1": 0}


def _cp(T):
    """A convex Cp(T) near the deck's: the chords of neighbouring segments
    differ by far more than rounding, and tables with knots that differ a
    little give almost the same temperatures."""
    return 1004.5 + 2.0e-4 * (T - 250.0) ** 2


def _common_quantiles(Ta, Tb, nk=8):
    """nk knots among the values of Ta and Tb such that every segment and both
    ends hold at least m values of Ta and m of Tb, for the largest such m."""
    Ta, Tb = np.sort(Ta), np.sort(Tb)
    cand = np.unique(np.concatenate([Ta, Tb]))
    for m in range(min(len(Ta), len(Tb)) // (nk + 1), 0, -1):
        # (a value equal to the first knot belongs to the lower end, one equal
        # to a later knot to the segment above it: segment())
        ks, na, nb = [], 0, 0   # values in the segments below the last knot
        for v in cand:
            side = "left" if ks else "right"
            ca, cb = int(np.searchsorted(Ta, v, side)), int(np.searchsorted(Tb, v, side))
            if ca - na >= m and cb - nb >= m:
                ks.append(float(v))
                na, nb = ca, cb
                if len(ks) == nk:
                    break
        if len(ks) == nk and len(Ta) - np.searchsorted(Ta, ks[-1], "left") >= m \
                and len(Tb) - np.searchsorted(Tb, ks[-1], "left") >= m:
            return ks
    raise AssertionError("no common quantiles")


@functools.lru_cache(maxsize=None)
def table_deck(text, kind):
    """text with Cp_air replaced by _cp at the kind's knots; returns (text,
    rows).  quantile8: knots at common quantiles of the gas cells' temperature
    in the first and in the last state of the CPU reference -- that of the
    unchanged deck, then, once more, that of the deck with those knots, whose
    temperatures are those of the final table to within its chord error."""
    gas = _gas(text)
    src = text
    for _ in range(2 if kind == "quantile8" else 1):
        ref = _cpu_reference(src)
        Ta, Tb = ref[0]["T"][gas].ravel(), ref[-1]["T"][gas].ravel()
        if kind == "quantile8":
            xs = _common_quantiles(Ta, Tb)
        elif kind == "n17":
            xs = [float(v) for v in np.linspace(min(Ta.min(), Tb.min()), max(Ta.max(), Tb.max()), 17)]
        else:
            xs = [float(np.median(Ta))]
        assert all(b > a for a, b in zip(xs, xs[1:])), xs
        rows = tuple((v, _cp(v)) for v in xs)
        src = decks.set_table(text, "Cp_air", rows)
    return src, rows


def assert_all_segments_hit(ref, rows, gas):
    """Every one of the table's segments and both extrapolating ends holds a
    gas cell in the first and in the last state of the CPU reference."""
    xs = [r[0] for r in rows]
    for snap in (ref[0], ref[-1]):
        hit = np.bincount(segment(xs, snap["T"][gas]), minlength=len(xs) + 1)
        assert (hit > 0).all(), hit


def _gas(text):
    import openhyperflow2d_amd as hf

    c = hf.Simulation(text, "cpu", lean=False)
    return np.asarray(c.field("solid")) == 0.0


def _tile_cases():
    import openhyperflow2d_amd as hf

    nat = hf.native()
    out = []
    for nt, cpt, tj, tj0 in GEOMS:
        for ny in (tj0 + 1, 2 * tj0 + 1):
            TI = nat.lean_tile_geom(100, ny, nt, tj, cpt)["TI"]
            for kind in KINDS:
                out.append((nt, cpt, tj, max(TI - 1, MIN_NX), ny, kind))
    return out


@pytest.mark.parametrize("nt,cpt,tj,nx,ny,kind", _tile_cases())
def test_tile_table_paths_match_cpu(gpu, monkeypatch, nt, cpt, tj, nx, ny, kind):
    text, rows = table_deck(sweep_deck(nx, ny), kind)
    if kind == "quantile8":
        assert_all_segments_hit(_cpu_reference(text), rows, _gas(text))
    g = _gpu(gpu, monkeypatch, text)
    sv = g.solver
    assert sv.lean_ok and sv.lean_sg_ok, sv.lean_why
    sv.cu_count = 0   # no two-cells-per-thread gate
    sv.lean_nt, sv.lean_cpt, sv.lean_tj = nt, cpt, tj
    nat = gpu.native()
    assert nat.air_table_build([r[0] for r in rows], [r[1] for r in rows])["mode"] == KINDS[kind]
    T = nat.lean_tile_geom(nx, ny, nt, tj, cpt)
    lasts = _march(g, text)
    assert lasts[0]["nt"] == 0, lasts[0]   # one step after the upload: the flat entry kernel
    seen = 0
    for last in lasts[1:]:
        assert (last["nt"], last["cpt"]) == (nt, cpt), last
        assert (last["TI"], last["TJ"], last["nbi"], last["nbj"]) == (T["TI"], T["TJ"], T["nbi"], T["nbj"]), last
        assert last["table"] == KINDS[kind], last
        seen |= last["seen"]
    assert seen == 7, seen   # plain, outputs and residual launches


def test_tile_table_fused_exchange_strips(gpu, monkeypatch):
    """hf2d_lean_tile_fx_nt at (64, 1, 16) with the quantile table: two strips
    on virtual ranks, interior tiles staged in a batch, edge tiles -- and
    their AirTable -- beside the mailbox columns == the CPU stepper."""
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text, rows = table_deck(decks.wedge15(48, 33, **BIG), "quantile8")
    ref = _cpu_reference(text)
    assert_all_segments_hit(ref, rows, _gas(text))
    held = {}

    def setup(s):
        s.cu_count = 0
        s.lean_nt, s.lean_cpt, s.lean_tj = 64, 1, 16

    def hook(k, solvers):
        held["solvers"] = solvers

    got, summ = _virtual_ranks(gpu, text, 2, SCHEDULE, lean=True, p2p=True, fuse=True, setup=setup,
                               chunk_hook=hook, case_hook=lambda c: perturb(c, SEED), fields=FIELDS)
    nat = gpu.native()
    for s in held["solvers"]:
        last = dict(s.lean_tile_last)
        assert (last["nt"], last["cpt"], last["TJ"], last["fx"], last["var"]) == (64, 1, 16, 1, 2), last
        assert last["table"] == 1, last
        T = nat.lean_tile_geom(last["nbi"] * last["TI"], 33, 64, 16, 1)
        assert last["nbi"] >= 3, last   # interior tile columns between the two edge ones
        assert last["stage"] == expected_stage(nat, 64, 1, T), last
        assert last["seen"] & 1, last   # plain fused steps too
    _assert_equal(lambda f: got[f], summ, ref[-1], True)
