"""The lean tile kernels at the shapes and variants the rest of the GPU suite
never reaches, from a start in which every cell differs from its neighbours
(tests/perturb.py), against the plain per-cell CPU stepper
(Simulation(text, "cpu", lean=False): no tiling code at all):

a. the headline variant -- 256 threads, two cells per thread, staggered
   start -- which DeviceSolver::do_step only picks for grids of at least
   2 * cu_count tiles (about 260 000 cells on the MI355X; cu_count is lowered
   here), single gas and 3-gas, plain / outputs / residual, eager and in step
   graphs, and with the mailbox exchange fused in (hf2d_lean_tile_fx);
b. a sweep of tile geometries and grid sizes at the edges of the tiling;
c. the lean N-S and lean mechanism tiles on the smallest decks with two tile
   columns and a partial last tile in both directions.

Every test asserts through DeviceSolver.lean_tile_last (or the lean step
counters) that the kernel it names really ran, and on the CPU reference that
no cell is flat at the start and at most 2 % are at the end."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from tests.perturb import FIELDS, SCHEDULE, flat_fraction, perturb, shape_sweep, sweep_deck

pytestmark = pytest.mark.gpu

SEED = 1
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
# graph windows start at multiples of 6 steps and need 6 plain steps: the
# schedule alone never fills one, so the graph cases run one longer call more
GRAPH_TAIL = [(26, False)]


@functools.lru_cache(maxsize=None)
def _cpu_reference(text, schedule=tuple(SCHEDULE), fields=tuple(FIELDS)):
    """Snapshots of the generic CPU stepper after every call of the schedule
    (computed once per deck, shared, never modified)."""
    import openhyperflow2d_amd as hf

    c = hf.Simulation(text, "cpu", lean=False)
    perturb(c, SEED)
    assert flat_fraction(c) == 0.0
    snaps = []
    for n, res in schedule:
        c.step(n, residual=res)
        s = dict(c.summary())
        snap = {"dt": s["dt"], "time": s["time"], "rms": np.array(s["rms"])}
        for f in fields:
            a = c.field(f).copy()
            a.setflags(write=False)
            snap[f] = a
        snaps.append(snap)
    gas = c.field("solid") == 0.0
    assert all(np.isfinite(snaps[-1][f][gas]).all() for f in fields)
    assert flat_fraction(c) <= 0.02
    return tuple(snaps)


def _assert_equal(g_fields, summ, snap, res, fields=FIELDS):
    assert summ["dt"] == snap["dt"]
    assert summ["time"] == snap["time"]
    if res:   # residual sums are reduced in another order on the device
        np.testing.assert_allclose(summ["rms"], snap["rms"], rtol=1e-12, atol=0)
    for f in fields:
        np.testing.assert_array_equal(g_fields(f), snap[f], err_msg=f)


def _march(g, text, schedule=SCHEDULE):
    """Run the schedule on the GPU simulation g, compare with the CPU
    reference after every call; returns lean_tile_last after every call."""
    ref = _cpu_reference(text, tuple(schedule))
    lasts = []
    for (n, res), snap in zip(schedule, ref):
        g.step(n, residual=res)
        lasts.append(dict(g.solver.lean_tile_last))
        _assert_equal(g.field, g.summary(), snap, res)
    return lasts


def _gpu(gpu, monkeypatch, text):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    g = gpu.Simulation(text, "gpu")
    perturb(g, SEED)
    return g


# --- a. the headline variant -------------------------------------------------

@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("deck", ["wedge", "triple_point"])
def test_headline_two_cell_tile_matches_cpu(gpu, monkeypatch, deck, graphs):
    """hf2d_lean_tile<..., SG, CPT = 2> at 256 threads (multi-gas: the 3-gas
    triple point), its plain, outputs and residual variants, with the
    staggered start (single gas) -- == the CPU stepper bit for bit."""
    text = decks.wedge15(221, 41, **BIG) if deck == "wedge" else decks.triple_point(160, 51, **BIG)
    g = _gpu(gpu, monkeypatch, text)
    sv = g.solver
    assert sv.lean_ok, sv.lean_why
    assert sv.lean_sg_ok == (deck == "wedge")
    sv.cu_count = 8
    sv.lean_nt, sv.lean_cpt, sv.lean_tj = 256, 2, 0
    sv.use_graph = graphs
    nx, ny = g.shape
    T = gpu.native().lean_tile_geom(nx, ny, 256, 0, 2)
    assert 16 <= T["nbi"] * T["nbj"] <= 32, T
    sched = SCHEDULE + (GRAPH_TAIL if graphs else [])
    lasts = _march(g, text, sched)
    seen = 0
    for (n, res), last in zip(sched, lasts):
        if n == 1:   # a download precedes every call: its first step is the flat re-entry kernel
            assert last["nt"] == 0, last
            continue
        assert (last["nt"], last["cpt"], last["fx"]) == (256, 2, 0), last
        assert (last["TI"], last["TJ"], last["nbi"], last["nbj"]) == (T["TI"], T["TJ"], T["nbi"], T["nbj"]), last
        assert last["var"] == (2 if res else 1), last
        assert (last["stagger"] != 0) == (deck == "wedge"), last
        seen |= last["seen"]
    assert seen == 7, seen   # plain, outputs and residual launches, all at cpt 2
    assert (sv.graph_launches > 1) == graphs


@pytest.mark.parametrize("nranks", [2, 3])
def test_headline_two_cell_tile_fused_exchange_strips(gpu, monkeypatch, nranks):
    """hf2d_lean_tile_fx at CPT = 2: strips on virtual ranks with the mailbox
    exchange fused into the two-cell tile kernel == the CPU stepper."""
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(240, 60, **BIG)
    ref = _cpu_reference(text)
    held = {}

    def setup(s):
        s.cu_count = 2
        s.lean_nt, s.lean_cpt, s.lean_tj = 256, 2, 0

    def hook(k, solvers):
        held["solvers"] = solvers

    got, summ = _virtual_ranks(gpu, text, nranks, SCHEDULE, lean=True, p2p=True, fuse=True, setup=setup,
                               chunk_hook=hook, case_hook=lambda c: perturb(c, SEED), fields=FIELDS)
    for s in held["solvers"]:
        last = dict(s.lean_tile_last)
        assert (last["nt"], last["cpt"], last["fx"], last["var"]) == (256, 2, 1, 2), last
        assert last["nbi"] * last["nbj"] >= 2 * s.cu_count, last
        assert last["seen"] & 1, last   # plain fused steps too
    _assert_equal(lambda f: got[f], summ, ref[-1], True)


# --- b. shape sweep ----------------------------------------------------------

def _sweep():
    import openhyperflow2d_amd as hf

    return shape_sweep(hf.native())


@pytest.mark.parametrize("nt,cpt,tj,nx,ny,top", _sweep())
def test_tile_shape_sweep_matches_cpu(gpu, monkeypatch, nt, cpt, tj, nx, ny, top):
    """Tile geometries x grid sizes at the edges of the tiling (one and two
    tile rows, a one-cell-high last row, strips narrower than a tile, TI = 1,
    idle threads, a live last grid row): xcd_remap, tile_of_part, the block
    dt reduction, the residual partials and the host-mirror tail at shapes
    nothing else runs."""
    text = sweep_deck(nx, ny, top)
    g = _gpu(gpu, monkeypatch, text)
    sv = g.solver
    assert sv.lean_ok and sv.lean_sg_ok, sv.lean_why
    sv.cu_count = 0   # no two-cells-per-thread gate
    sv.lean_nt, sv.lean_cpt, sv.lean_tj = nt, cpt, tj
    T = gpu.native().lean_tile_geom(nx, ny, nt, tj, cpt)
    lasts = _march(g, text)
    assert lasts[0]["nt"] == 0, lasts[0]   # one step after the upload: the flat entry kernel
    seen = 0
    for (n, res), last in list(zip(SCHEDULE, lasts))[1:]:
        assert (last["nt"], last["cpt"]) == (nt, cpt), last
        assert (last["TI"], last["TJ"], last["nbi"], last["nbj"]) == (T["TI"], T["TJ"], T["nbi"], T["nbj"]), last
        seen |= last["seen"]
    assert seen == 7, seen


def test_grid_lower_than_a_tile_runs_the_flat_kernel(gpu, monkeypatch):
    """ny = 7 < LEAN_TILE_MIN_TJ: no tile launch, and the flat lean kernel
    equals the CPU stepper too."""
    text = decks.wedge15(40, 7, **BIG)
    g = _gpu(gpu, monkeypatch, text)
    assert g.solver.lean_ok, g.solver.lean_why
    lasts = _march(g, text)
    assert all(last["nt"] == 0 for last in lasts), lasts


# --- c. lean N-S and lean mechanism tiles ------------------------------------

NS_FIELDS = FIELDS + ["mu", "lam", "mu_t", "S7", "S8"]


def _lean_vs_split(gpu, monkeypatch, text, fields, configure, steps_of):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    c = gpu.Simulation(text, "cpu", lean=False)
    perturb(c, SEED)
    assert flat_fraction(c) == 0.0
    a = gpu.Simulation(text, "gpu")
    b = gpu.Simulation(text, "gpu")
    for s in (a, b):
        perturb(s, SEED)
        s.solver.use_graph = False
    configure(a.solver, b.solver)
    for n, res in SCHEDULE:
        a.step(n, residual=res)
        b.step(n, residual=res)
        c.step(n, residual=res)
        assert a.summary()["dt"] == b.summary()["dt"]
        assert abs(a.summary()["dt"] / c.summary()["dt"] - 1) <= 1e-9
    assert steps_of(a.solver) > 0 and steps_of(b.solver) == 0
    assert a.summary()["time"] == b.summary()["time"]
    np.testing.assert_allclose(a.summary()["rms"], b.summary()["rms"], rtol=1e-12, atol=0)
    for f in fields:
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)
    ra = np.frombuffer(a.records(), dtype=np.float64).reshape(-1, 156).copy()
    rb = np.frombuffer(b.records(), dtype=np.float64).reshape(-1, 156).copy()
    assert (np.isnan(ra) == np.isnan(rb)).all()
    ra[np.isnan(ra)] = 0
    rb[np.isnan(rb)] = 0
    np.testing.assert_array_equal(ra.view(np.uint64), rb.view(np.uint64))
    gas = c.field("solid") == 0.0
    for f in ["rho", "U", "V", "p", "T"]:
        x, y = a.field(f), c.field(f)
        assert np.isfinite(y[gas]).all(), f
        assert np.abs(x - y)[gas].max() <= 1e-9 * np.abs(y[gas]).max(), f
    assert flat_fraction(c) <= 0.02


@pytest.mark.parametrize("tj", [0, 8, 16])
@pytest.mark.parametrize("deck", ["step", "resonator"])
def test_lean_ns_small_tiles(gpu, monkeypatch, deck, tj):
    """hf2d_lns_step* (laminar step, k-eps resonator) on 37 x 23 cells: with
    16-row tiles two full tile columns and five more columns, one full tile
    row and seven more rows (tj = 8: 32-column tiles, three tile rows; 0: the
    kernel's own choice) -- lean == split bitwise on the GPU, GPU == CPU to
    1e-9."""
    text = (decks.step if deck == "step" else decks.resonator)(37, 23, **BIG)
    if tj:
        T = gpu.native().lean_tile_geom(37, 23, 256, tj, 1)
        assert T["nbi"] >= 2 and 37 % T["TI"] and 23 % T["TJ"], T

    def configure(a, b):
        assert a.lns_ok, a.lns_why
        a.lean_tj = b.lean_tj = tj
        b.lean_ns = False

    _lean_vs_split(gpu, monkeypatch, text, NS_FIELDS, configure, lambda s: s.lns_steps)


@pytest.mark.parametrize("ti", [16, 12])
def test_lean_mech_small_tiles(gpu, monkeypatch, ti):
    """hf2d_lnm_step on a 37 x 23 scramjet with the H2/air mechanism: 16-row
    tiles of 16 (the default) or 12 columns, a partial last tile in both
    directions -- lean == split bitwise on the GPU, GPU == CPU to 1e-9."""
    text = decks.scramjet(37, 23, **BIG)

    def configure(a, b):
        assert a.lnm_ok, a.lnm_why
        assert a.lnm_ti == 16
        a.lnm_ti = ti
        b.lean_mech = False

    _lean_vs_split(gpu, monkeypatch, text, NS_FIELDS + ["Y:H2", "Y:O2", "Y:OH", "Y:H2O", "Y:N2"], configure,
                   lambda s: s.lnm_steps)


# --- step graphs and the settings a captured window bakes in ------------------

def test_graph_windows_follow_changed_settings(gpu, monkeypatch):
    """A cached step graph must not replay after dt_read_mode or cu_count
    changed (DeviceSolver::mode_signature): the next window is captured anew
    with the new setting, and the run equals solvers that had the setting from
    the start, and the CPU stepper."""
    text = decks.wedge15(221, 41, **BIG)
    a, b, c = [_gpu(gpu, monkeypatch, text) for _ in range(3)]
    for r in (a, b, c):
        r.solver.use_graph = True
        r.solver.lean_nt, r.solver.lean_cpt, r.solver.lean_tj = 256, 2, 0
        r.solver.cu_count = 8
    b.solver.dt_read_mode = c.solver.dt_read_mode = 2
    c.solver.cu_count = 256   # 20 tiles are fewer than two per CU: one cell per thread
    calls = [(24, False)] * 3   # (24 steps: windows at steps 6 and 12, replayed or captured anew)
    for r in (a, b, c):
        r.step(24)
    caps = [r.solver.graph_captures for r in (a, b, c)]
    assert min(caps) > 0 and a.solver.graph_launches > caps[0], (caps, a.solver.graph_launches)
    assert a.solver.lean_tile_last["dt_read"] == 1 and b.solver.lean_tile_last["dt_read"] == 2
    assert a.solver.lean_tile_last["cpt"] == 2 and c.solver.lean_tile_last["cpt"] == 1
    a.solver.dt_read_mode = 2
    for r in (a, b, c):
        r.step(24)
    assert a.solver.graph_captures == caps[0] + 1, a.solver.graph_captures
    assert [b.solver.graph_captures, c.solver.graph_captures] == caps[1:]   # unchanged settings: replays
    assert a.solver.lean_tile_last["dt_read"] == 2, a.solver.lean_tile_last
    a.solver.cu_count = 256
    for r in (a, b, c):
        r.step(24)
    assert a.solver.graph_captures == caps[0] + 2, a.solver.graph_captures
    assert [b.solver.graph_captures, c.solver.graph_captures] == caps[1:]
    assert a.solver.lean_tile_last["cpt"] == 1, a.solver.lean_tile_last
    assert a.summary()["dt"] == b.summary()["dt"] == c.summary()["dt"]
    for f in FIELDS:
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)
        np.testing.assert_array_equal(a.field(f), c.field(f), err_msg=f)
    _assert_equal(a.field, a.summary(), _cpu_reference(text, tuple(calls))[-1], False)


def test_graph_windows_follow_a_knob_the_old_list_missed(gpu, monkeypatch):
    """tile_stagger is an argument of the captured tile launches (every `graph`
    row of the knob table is part of DeviceSolver::mode_signature): after it
    changes, exactly one window is captured anew and carries the new start
    delay, and the run equals a solver that had it from the start bit for bit."""
    text = decks.wedge15(221, 41, **BIG)
    a, b = [_gpu(gpu, monkeypatch, text) for _ in range(2)]
    for r in (a, b):
        r.solver.use_graph = True
        r.solver.lean_nt, r.solver.lean_cpt, r.solver.lean_tj = 256, 2, 0
        r.solver.cu_count = 8   # 20 two-cell tiles: at least two per CU, at most four rounds (the stagger gate)
    a.solver.tile_stagger = 0
    b.solver.tile_stagger = 150
    for r in (a, b):
        r.step(24)
    caps = [r.solver.graph_captures for r in (a, b)]
    assert min(caps) > 0 and a.solver.graph_launches > caps[0], (caps, a.solver.graph_launches)
    assert a.solver.lean_tile_last["stagger"] == 0 and b.solver.lean_tile_last["stagger"] == 150
    a.solver.tile_stagger = 150
    for r in (a, b):
        r.step(24)
    assert a.solver.graph_captures == caps[0] + 1, a.solver.graph_captures
    assert b.solver.graph_captures == caps[1]   # unchanged settings: replays
    assert a.solver.lean_tile_last["stagger"] == 150, a.solver.lean_tile_last
    assert (a.solver.lean_tile_last["nt"], a.solver.lean_tile_last["cpt"]) == (256, 2)
    assert a.summary()["dt"] == b.summary()["dt"]
    for f in FIELDS:
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)


def test_graph_windows_follow_fill_occ_on_the_split_path(gpu, monkeypatch):
    """The split predict / fill steps in step graphs (laminar step, 37 x 23,
    lean N-S off): fill_occ selects the fill kernel's pointer, so a change
    captures exactly one window anew, and the run equals a twin that had
    fill_occ = 2 from the start bit for bit."""
    text = decks.step(37, 23, **BIG)
    a, b = [_gpu(gpu, monkeypatch, text) for _ in range(2)]
    for r in (a, b):
        r.solver.lean_ns = False
        r.solver.use_graph = True
    assert a.solver.fill_occ == -1
    b.solver.fill_occ = 2
    for r in (a, b):
        r.step(24)
    caps = [r.solver.graph_captures for r in (a, b)]
    assert min(caps) > 0 and a.solver.graph_launches > caps[0], (caps, a.solver.graph_launches)
    assert a.solver.lns_steps == 0 and b.solver.lns_steps == 0
    a.solver.fill_occ = 2
    for r in (a, b):
        r.step(24)
    assert a.solver.graph_captures == caps[0] + 1, a.solver.graph_captures
    assert b.solver.graph_captures == caps[1]   # unchanged settings: replays
    assert a.solver.lns_steps == 0 and b.solver.lns_steps == 0
    assert a.summary()["dt"] == b.summary()["dt"]
    for f in NS_FIELDS:
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)
