"""Per-step frame recorder on the device (hf2d_wallq_tick / hf2d_frame_rows /
hf2d_frame_store, hip/frame_history.hpp): the ten FRAME_VARS on the cells of a
strided region, written by three launches at the end of every step from
whichever representation is authoritative -- generic record, lean inviscid
arrays, lean N-S levels (SGL / SGT), lean mechanism state.

The oracle is a twin simulation of the same backend and settings without a
recorder, advanced with step(1) and a download after every step, and read
through Case.frame (computed once per deck, shared, never modified).  Every
comparison is bitwise.  The decks, paths, schedules and path assertions are
those of test_gpu_probe_history.py; all runs start from tests.perturb.perturb.
Each case asserts through the solver's counters that the kernel it names ran,
and that recording changed neither the counters nor the final fields.  A solid
node entering a lean N-S / mechanism fill raises the step's error flag, which
the next step() call throws."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import FRAME_VARS, PROBE_VARS
from tests.perturb import SCHEDULE, perturb
from tests.test_frames import V, same_bits
from tests.test_gpu_probe_history import BIG, DECKS, GRAPH_SCHEDULE, SEED, _assert_path, _cells, _sim, _tile

pytestmark = pytest.mark.gpu

STATIC = ("vars", "i", "j", "x", "y", "gas")


@functools.lru_cache(maxsize=None)
def _twin(name, nsteps=52):
    """times [n], frames [n, 10, nx, ny] of the recorder-free twin after each of its one-step calls."""
    import openhyperflow2d_amd as hf

    s = _sim(hf, name, False)
    times, vals = [], []
    for _ in range(nsteps):
        s.step(1)
        s.solver.download()
        vals.append(np.asarray(s.case.frame()["values"]).copy())
        times.append(s.summary()["time"])
    out = np.array(times), np.array(vals)
    for a in out:
        a.setflags(write=False)
    return out


def _run(s, sched):
    for n, res in sched:
        s.step(n, residual=res)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_history_equals_the_twin(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _sim(gpu, name, graphs), _sim(gpu, name, graphs)
    a.record_frames(vars=FRAME_VARS, capacity=64)
    for n, res in sched:   # (a raised error flag -- a solid node in a lean fill -- would throw here)
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.frame_history()
    times, vals = _twin(name)
    assert h["total"] == nsteps and h["vars"] == FRAME_VARS and h["values"].dtype == np.float64
    for v, var in enumerate(FRAME_VARS):
        same_bits(h["values"][:, v], vals[:nsteps, v], "%s of %s" % (var, name))
    np.testing.assert_array_equal(h["times"], times[:nsteps])
    f = a.case.frame()
    for k in STATIC:
        np.testing.assert_array_equal(h[k], f[k], err_msg=k)
    gas = h["gas"]
    assert gas.any()
    # no comparison of constants
    g = vals[:nsteps, V["grad_rho"]][:, gas]
    assert (g[1:] != g[:-1]).any() and np.isfinite(g).all()
    # the named kernel ran, and recording left neither the lean state nor the graphs
    T = _tile(gpu, name, a.case.nx, a.case.ny)
    for s in (a, b):
        _assert_path(s.solver, name, T)
    assert (a.solver.graph_launches > 1) == graphs, a.solver.graph_launches
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(a.solver, k) == getattr(b.solver, k), k
    # reading the history moved nothing: the next steps and the final fields are the plain run's
    assert a.summary()["dt"] == b.summary()["dt"] and a.summary()["time"] == b.summary()["time"]
    for fld in PROBE_VARS + ("k", "CP"):
        np.testing.assert_array_equal(a.field(fld), b.field(fld), err_msg=fld)


def _assert_region(h, times, vals, rows, vars, region, stride, what=""):
    i0, i1, j0, j1 = region
    ii, jj = np.arange(i0, i1, stride[0]), np.arange(j0, j1, stride[1])
    np.testing.assert_array_equal(h["i"], ii, err_msg=what)
    np.testing.assert_array_equal(h["j"], jj, err_msg=what)
    assert h["values"].shape == (len(rows), len(vars), len(ii), len(jj)), (h["values"].shape, what)
    for k, var in enumerate(vars):
        same_bits(h["values"][:, k], vals[rows, V[var]][:, ii][:, :, jj], "%s %s" % (var, what))
    np.testing.assert_array_equal(h["times"], times[rows], err_msg=what)


def test_region_shapes(gpu, monkeypatch):
    """wedge15(67, 23), two tiles each way: one-cell regions at the gas corners, a column, a row, 255 and
    256 output cells, a region touching all four edges, strides; each armed on the running simulation
    (arming again replaces the recorder) and compared over the two steps that follow."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    name = "wedge_tile"
    times, vals = _twin(name)
    a = _sim(gpu, name, False)
    gas = np.asarray(a.case.frame(vars=("rho",))["gas"])
    nx, ny = gas.shape
    corners = []
    for i in (0, nx - 1):   # the lowest and the highest gas cell of the first and the last column
        free = np.flatnonzero(gas[i])
        corners += [(i, int(free[0])), (i, int(free[-1]))]
    assert len(set(corners)) == 4 and not gas.all()
    regions = [((i, i + 1, j, j + 1), (1, 1)) for i, j in corners]
    regions += [((33, 34, 0, ny), (1, 1)), ((0, nx, 11, 12), (1, 1)), ((20, 35, 3, 20), (1, 1)), ((40, 56, 5, 21), (1, 1)),
                ((0, nx, 0, ny), (1, 1)), ((0, nx, 0, ny), (2, 3)), ((1, nx, 0, ny - 1), (5, 1))]
    assert 15 * 17 == 255 and 16 * 16 == 256
    k = 0
    for region, stride in regions:
        a.record_frames(vars=FRAME_VARS, region=region, stride=stride, capacity=2)
        a.step(2)
        h = a.frame_history()
        assert h["total"] == 2
        _assert_region(h, times, vals, [k, k + 1], FRAME_VARS, region, stride, "%s %s" % (region, stride))
        k += 2
    assert k <= len(times)
    _assert_path(a.solver, name, _tile(gpu, name, nx, ny))


def test_a_257_cell_row(gpu, monkeypatch):
    """257 x 1 output cells on wedge15(260, 9): the store kernel's second workgroup holds one cell."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(260, 9, **BIG)
    a, b = gpu.Simulation(text, "gpu"), gpu.Simulation(text, "gpu")
    for s in (a, b):
        perturb(s, SEED)
    vars = ("grad_p", "vorticity", "T")
    region = (2, 259, 6, 7)
    a.record_frames(vars=vars, region=region, capacity=4)
    for k in range(3):
        a.step(1)
        b.step(1)
        b.solver.download()
        want = b.case.frame(vars=vars, region=region)
        h = a.frame_history()
        assert h["values"].shape == (k + 1, 3, 257, 1) and want["gas"].all()
        same_bits(h["values"][-1], want["values"], "step %d" % k)
        assert h["times"][-1] == b.summary()["time"]
    assert h["values"][:, 0].any()


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_ring_wraps_inside_graphs(gpu, monkeypatch, name):
    """every = 3, capacity = 4 across the 26-step call (graph windows): the last four samples, in order;
    then a cleared recorder."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    times, vals = _twin(name)
    a = _sim(gpu, name, True)
    a.record_frames(every=3, capacity=4)
    _run(a, GRAPH_SCHEDULE)
    assert a.solver.graph_launches > 1
    h = a.frame_history()
    rows = list(range(2, nsteps, 3))
    assert h["total"] == len(rows) == 13 and h["vars"] == ("rho", "grad_rho")
    whole = (0, a.case.nx, 0, a.case.ny)
    _assert_region(h, times, vals, rows[-4:], ("rho", "grad_rho"), whole, (1, 1), name)
    a.clear_frames()
    z = a.frame_history()
    assert z["total"] == 0 and z["values"].shape[0] == 0
    a.step(7)
    h = a.frame_history()
    assert h["total"] == 2
    _assert_region(h, times, vals, [nsteps + 2, nsteps + 5], ("rho", "grad_rho"), whole, (1, 1), name + " cleared")


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_arming_after_cached_windows(gpu, monkeypatch, name):
    """26 steps unarmed, arm, 26 more: the windows cached before arming must not replay."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    n = 26
    times, vals = _twin(name)
    a = _sim(gpu, name, True)
    a.step(n)
    before = a.solver.graph_launches
    assert before > 1
    vars = ("ducros", "U")
    a.record_frames(vars=vars, every=3, capacity=64)
    a.step(n)
    h = a.frame_history()
    assert len(times) == 52 and h["total"] == 8
    _assert_region(h, times, vals, list(range(n + 2, 2 * n, 3)), vars, (0, a.case.nx, 0, a.case.ny), (1, 1), name)
    assert a.solver.graph_launches > before + 1   # captured again with the recorder, then replayed


@pytest.mark.parametrize("name", ["wedge_generic", "wedge_flat", "wedge_tile", "triple_point"])
def test_gpu_recorder_equals_the_cpu_recorder(gpu, monkeypatch, name):
    """The inviscid decks: the CPU backend's recorder, frame for frame and bit for bit."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    gen, kw, _, _ = DECKS[name]
    g = _sim(gpu, name, False)
    c = gpu.Simulation(gen(), "cpu", **kw)
    perturb(c, SEED)
    for s in (g, c):
        s.record_frames(vars=FRAME_VARS, stride=(2, 1), every=2, capacity=64)
        _run(s, SCHEDULE)
    hg, hc = g.frame_history(), c.frame_history()
    assert hg["total"] == hc["total"] == 7 and hg.keys() == hc.keys()
    same_bits(hg["values"], hc["values"], name)
    for k in ("times",) + STATIC:
        np.testing.assert_array_equal(hg[k], hc[k], err_msg=k)


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_all_six_observers_at_once(gpu, monkeypatch, name):
    """Probes, averaging, loads, wall heat, the surface and the frames armed together: each history is
    that of its own single-observer run."""
    from tests.test_gpu_surface import _make
    from tests.test_load_history import targets

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    sims = [_make(gpu, name, True) for _ in range(7)]
    all6, probes, avg, loads, heat, surf, frames = sims
    cells, _ = _cells(gpu, all6, name)
    boxes, cuts = targets(all6.case)
    for s in (all6, probes):
        s.record_probes(cells, capacity=64)
    for s in (all6, avg):
        s.start_averaging()
    for s in (all6, loads):
        s.record_loads(boxes, cuts, capacity=64)
    for s in (all6, heat):
        s.record_wall_heat(capacity=64)
    for s in (all6, surf):
        s.record_surface(capacity=64)
    for s in (all6, frames):
        s.record_frames(vars=FRAME_VARS, every=2, capacity=64)
    for n, res in GRAPH_SCHEDULE:
        for s in sims:
            s.step(n, residual=res)
    fa, fb = all6.frame_history(), frames.frame_history()
    assert fa["total"] == fb["total"] == nsteps // 2 and fa["values"][:, V["grad_p"]].any()
    same_bits(fa["values"], fb["values"])
    np.testing.assert_array_equal(fa["times"], fb["times"])
    hp, hq = all6.probe_history(), probes.probe_history()
    np.testing.assert_array_equal(hp["values"], hq["values"])
    np.testing.assert_array_equal(hp["times"], hq["times"])
    np.testing.assert_array_equal(hp["times"][1::2], fa["times"])
    A, B = all6.averages(), avg.averages()
    assert A["samples"] == B["samples"] == nsteps and A["time"] == B["time"]
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(A[k], B[k], err_msg=k)
    la, lb = all6.load_history(), loads.load_history()
    for k in ("times", "forces", "mass_flow"):
        np.testing.assert_array_equal(la[k], lb[k], err_msg=k)
    for x, y in ((all6.wall_heat_history(), heat.wall_heat_history()), (all6.surface_history(), surf.surface_history())):
        for k in x:
            np.testing.assert_array_equal(x[k], y[k], err_msg=k)
    assert all6.solver.graph_launches > 1
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(all6.solver, k) == getattr(probes.solver, k), k


@pytest.mark.parametrize("p2p", [False, True], ids=["local", "p2p"])
@pytest.mark.parametrize("deck", ["wedge", "step"])
def test_strips_record_their_own_columns(gpu, monkeypatch, deck, p2p):
    """Three strips on virtual ranks: every rank's row variables, placed by its `i`, together are the
    one-GPU history; a gradient variable refuses and leaves the armed recorder intact."""
    from openhyperflow2d_amd.parallel.strips import balanced_columns
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(120, 30, **BIG) if deck == "wedge" else decks.step(120, 30, **BIG)
    ref = gpu.Simulation(text, "gpu")
    perturb(ref, SEED)
    solid = ref.field("solid")
    parts = balanced_columns(solid, 3)
    args = dict(vars=list(PROBE_VARS), region=(1, 119, 2, 29), stride=(2, 3), every=2, capacity=4)
    ref.record_frames(**args)
    _run(ref, SCHEDULE)
    one = ref.frame_history()
    held, stats = [], {}

    def setup(s):
        held.append(s)
        s.record_frames(args["vars"], args["region"], args["stride"], args["every"], args["capacity"])
        with pytest.raises(RuntimeError, match="strip"):
            s.record_frames(["rho", "grad_rho"])

    _virtual_ranks(gpu, text, 3, SCHEDULE, lean=True, p2p=p2p, setup=setup, parts=parts,
                   case_hook=lambda c: perturb(c, SEED), stats=stats)
    if deck == "step":
        assert min(stats["lns_steps"]) > 0 and ref.solver.lns_steps > 0, stats
    assert one["total"] == 7 and one["values"].shape[0] == 4 and one["values"][:, 2].any()
    got = np.full_like(one["values"], np.nan)
    seen = []
    for s, (a, b) in zip(held, parts):
        h = dict(s.frame_history())
        cols = np.asarray(h["i"])
        assert cols.tolist() == [i for i in one["i"].tolist() if a <= i < b] and tuple(h["vars"]) == PROBE_VARS
        assert int(h["total"]) == 7
        np.testing.assert_array_equal(np.asarray(h["times"]), one["times"])
        np.testing.assert_array_equal(np.asarray(h["j"]), one["j"])
        at = np.searchsorted(one["i"], cols)
        got[:, :, at, :] = np.asarray(h["values"])
        np.testing.assert_array_equal(np.asarray(h["gas"]), one["gas"][at])
        seen += cols.tolist()
    assert seen == one["i"].tolist()
    same_bits(got, one["values"])


def test_frames_across_a_cycle_match_cpu(gpu, tmp_path):
    """DeviceSolver::on_cycle_roll() moves the frame ring's stored times with the device's time_part and
    the offset of the recorder's clock.  Armed before run() on the deck and march of
    test_gpu_model_families (cycle boundary after step 30 of 43): every frame equals the CPU recorder's
    bit for bit, the times after the boundary too; a time of the cycle before it is converted as
    global_time + (t_row - t_roll), two roundings of at most half an ulp of the boundary's time each."""
    from tests import model_families as mf

    row = mf.BY_ID["bff_linear"]
    g, c = mf.simulation(gpu, row, "gpu"), mf.simulation(gpu, row, "cpu", lean=False)
    out = []
    for s in (g, c):
        s.record_frames(vars=FRAME_VARS, stride=(3, 2), every=2, capacity=64)
        assert list(mf.march(s, tmp_path)) == [0, 1, 2, 3]
        out.append((s.frame_history(), s.summary()))
    (hg, sg), (hc, sc) = out
    assert sg["time"] == sc["time"] and sg["iteration"] == sc["iteration"] == 43
    assert hg["total"] == hc["total"] == 21
    same_bits(hg["values"], hc["values"])
    np.testing.assert_array_equal(hg["times"][15:], hc["times"][15:])
    t_roll = hc["times"][14]   # (sample 15 is step 30, the last of the first cycle)
    assert np.abs(hg["times"][:15] - hc["times"][:15]).max() <= np.spacing(t_roll)
    assert (np.diff(hg["times"]) > 0).all() and hg["values"][:, V["grad_rho"]].any()
