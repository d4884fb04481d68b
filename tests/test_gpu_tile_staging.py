"""The two staging forms of the single-gas lean tile kernels -- all of a
thread's slots loaded in one batch (lean_tile.hpp: lean_stage_issue /
lean_stage_write) or the loop of lean_tile_stage -- at tile geometries on both
sides of the batch limit, from a start in which every cell differs from its
neighbours (tests/perturb.py), against the plain per-cell CPU stepper, bit for
bit after every call of the schedule.

A thread stages K = ceil(NC / nt) slots of the tile and its halo; the kernel
of nt threads and cpt cells per thread batches up to
native.lean_tile_stage_kmax(nt, cpt) of them and runs the loop beyond.  Every
case asserts through DeviceSolver.lean_tile_last that the named geometry ran
and which staging it took; the reference conditions (no flat cell at the
start, at most 2 % at the end, all gas cells finite) are those of
test_gpu_tile_shapes.py."""
import pytest

from openhyperflow2d_amd.models import decks
from tests.perturb import FIELDS, MAX_CELLS, MIN_NX, SCHEDULE, perturb, sweep_deck
from tests.test_gpu_tile_shapes import BIG, SEED, _assert_equal, _cpu_reference, _gpu, _march

pytestmark = pytest.mark.gpu

# (threads per workgroup, cells per thread, tile height override, tile height
# of the lowest grid): the headline's (64, 1, 16), K = 2; (64, 1, 32), K = 3;
# (64, 1, 64), K = 4; tj = 0: the kernel's own height, which is ny up to 32
GEOMS = [(64, 1, 16, 16), (128, 1, 8, 8), (64, 1, 8, 8), (64, 1, 32, 32), (64, 1, 64, 64), (256, 2, 0, 32),
         (256, 1, 0, 32)]


def slots_per_thread(T, nt):
    return (T["NC"] + nt - 1) // nt


def staging_cases(native):
    """[(nt, cpt, tj, nx, ny, top)]: every geometry at ny = TJ (one tile row),
    TJ + 1 (a one-cell last row) and 2 TJ + 1 (three rows), each at
    nx = max(TI - 1, MIN_NX) (a partial last tile), the first multiple of TI
    from MIN_NX on (an exact one) and that + 1 (a one-column last tile);
    tilings of more than one tile row once more, at the last nx, with the open
    top boundary."""
    seen, out = set(), []
    for nt, cpt, tj, tj0 in GEOMS:
        for ny in (tj0, tj0 + 1, 2 * tj0 + 1):
            TI = native.lean_tile_geom(100, ny, nt, tj, cpt)["TI"]
            exact = -(-MIN_NX // TI) * TI
            for nx, top in [(max(TI - 1, MIN_NX), "farfield"), (exact, "farfield"), (exact + 1, "farfield"),
                            (exact + 1, "open")]:
                g = native.lean_tile_geom(nx, ny, nt, tj, cpt)
                key = (nt, cpt, tj, nx, ny, top)
                if key in seen or (top == "open" and g["nbj"] < 2):
                    continue
                assert nx * ny <= MAX_CELLS, key
                seen.add(key)
                out.append(key)
    return out


def expected_stage(native, nt, cpt, T):
    K = slots_per_thread(T, nt)
    return K if K <= native.lean_tile_stage_kmax(nt, cpt) else 0


def _cases():
    import openhyperflow2d_amd as hf

    nat = hf.native()
    cases = staging_cases(nat)
    stages = {expected_stage(nat, nt, cpt, nat.lean_tile_geom(nx, ny, nt, tj, cpt))
              for nt, cpt, tj, nx, ny, top in cases}
    # both forms must be under test, whatever the batch limits are
    if 0 not in stages or not (stages - {0}):
        raise RuntimeError("staging cases cover one staging form only: %s" % sorted(stages))
    return cases


@pytest.mark.parametrize("nt,cpt,tj,nx,ny,top", _cases())
def test_tile_staging_matches_cpu(gpu, monkeypatch, nt, cpt, tj, nx, ny, top):
    """Batched and looped staging at partial, exact and one-column last tiles,
    one, two (one-cell) and three tile rows == the CPU stepper bit for bit."""
    text = sweep_deck(nx, ny, top)
    g = _gpu(gpu, monkeypatch, text)
    sv = g.solver
    assert sv.lean_ok and sv.lean_sg_ok, sv.lean_why
    sv.cu_count = 0   # no two-cells-per-thread gate
    sv.lean_nt, sv.lean_cpt, sv.lean_tj = nt, cpt, tj
    nat = gpu.native()
    T = nat.lean_tile_geom(nx, ny, nt, tj, cpt)
    stage = expected_stage(nat, nt, cpt, T)
    lasts = _march(g, text)
    assert lasts[0]["nt"] == 0, lasts[0]   # one step after the upload: the flat entry kernel
    seen = 0
    for last in lasts[1:]:
        assert (last["nt"], last["cpt"]) == (nt, cpt), last
        assert (last["TI"], last["TJ"], last["nbi"], last["nbj"]) == (T["TI"], T["TJ"], T["nbi"], T["nbj"]), last
        assert last["stage"] == stage, (last, slots_per_thread(T, nt))
        seen |= last["seen"]
    assert seen == 7, seen   # plain, outputs and residual launches


def test_tile_staging_fused_exchange_strips(gpu, monkeypatch):
    """hf2d_lean_tile_fx_nt at the headline's (64, 1, 16): two strips on
    virtual ranks, the mailbox exchange fused into the tile kernel -- interior
    tiles staged in a batch, edge tiles from the mailbox -- == the CPU
    stepper."""
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(48, 33, **BIG)
    ref = _cpu_reference(text)
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
        T = nat.lean_tile_geom(last["nbi"] * last["TI"], 33, 64, 16, 1)
        assert last["nbi"] >= 3, last   # interior tile columns between the two edge ones
        assert last["stage"] == expected_stage(nat, 64, 1, T), last
        assert last["seen"] & 1, last   # plain fused steps too
    _assert_equal(lambda f: got[f], summ, ref[-1], True)
