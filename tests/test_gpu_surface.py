"""Per-step surface recorder on the device (hf2d_wallq_tick / hf2d_surf_cells /
hf2d_surf_nodes, hip/surface_history.hpp): p, Cp, T, tau_x, tau_y, Cf_x, Cf_y,
q_y, q_x and St of every wall node and their running statistics, written by
three launches at the end of every step from whichever representation is
authoritative -- generic record, lean inviscid arrays, lean N-S levels (SGL /
SGT), lean mechanism state.

The oracle is a twin simulation of the same backend and settings without a
recorder, advanced with step(1) and a download after every step, and read
through Case.surface (computed once per deck, shared, never modified); the
statistics' oracle is the rule transcribed in NumPy
(tests.test_surface.stats_oracle) over the twin's values and times.  Every
comparison is bitwise.  The decks, paths and schedules are those of
test_gpu_probe_history.py with the heat-flux keys set; all runs start from
tests.perturb.perturb.  Each case asserts through the solver's counters that
the kernel it names ran, and that recording changed neither the counters nor
the final fields."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.perturb import SCHEDULE, perturb
from tests.test_gpu_probe_history import BIG, DECKS, GRAPH_SCHEDULE, SEED, _assert_path, _cells, _tile
from tests.test_gpu_wall_heat import LONG
from tests.test_load_history import targets
from tests.test_surface import V, assert_history, assert_stats, assert_table, make_twin, stats_oracle
from tests.test_wall_heat import heat_keys

pytestmark = pytest.mark.gpu

EDGES = (0, 1, 64, 65, 256, 257)   # nodes of the lists around the wavefront's and the workgroup's size


def _make(gpu, name, graphs, backend="gpu"):
    """test_gpu_probe_history._sim with the heat-flux keys set on the deck."""
    gen, kw, attrs = DECKS[name][:3] if name in DECKS else (LONG[name][0], {}, {})
    s = gpu.Simulation(heat_keys(gen()), backend, **(kw if backend == "gpu" else {}))
    perturb(s, SEED)
    if backend == "gpu":
        for k, v in attrs.items():
            setattr(s.solver, k, v)
        s.solver.use_graph = graphs
    return s


@functools.lru_cache(maxsize=None)
def _twin(name, nsteps=52):
    """times [n], values [n, 10, nnodes] of the recorder-free twin after each of its one-step calls."""
    import openhyperflow2d_amd as hf

    return make_twin(_make(hf, name, False), nsteps)


def _assert_not_constant(name, vals, n):
    """A comparison of constants proves nothing: p, tau_x and q_y of the twin vary over the run.  The
    wedge decks are Euler decks: their viscosity and hence every tau_x is zero at every step, which is
    asserted instead."""
    if name == "triple_point":   # no node
        assert vals.shape[2] == 0
        return
    for q in ("p", "q_y"):
        assert (vals[1:n, V[q]] != vals[:n - 1, V[q]]).any(), (name, q)
    if name.startswith("wedge"):
        assert not vals[:n, V["tau_x"]].any()
    else:
        assert (vals[1:n, V["tau_x"]] != vals[:n - 1, V["tau_x"]]).any(), name


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_history_equals_the_twin(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _make(gpu, name, graphs), _make(gpu, name, graphs)
    a.record_surface(capacity=64)
    for n, res in sched:
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.surface_history()
    times, vals = _twin(name)
    assert h["total"] == nsteps
    assert_history(h, times, vals, range(nsteps), name)
    assert_stats(h, stats_oracle(times, vals, 0.0, hi=nsteps), name)
    _assert_not_constant(name, vals, nsteps)
    assert_table(h, a.case.surface(), name)
    assert (len(h["i"]) > 0) == (name != "triple_point")
    # the named kernel ran, and recording left neither the lean state nor the graphs
    T = _tile(gpu, name, a.case.nx, a.case.ny)
    for s in (a, b):
        _assert_path(s.solver, name, T)
    assert (a.solver.graph_launches > 1) == graphs, a.solver.graph_launches
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(a.solver, k) == getattr(b.solver, k), k
    # reading the history moved nothing: the next steps and the final fields are the plain run's
    assert a.summary()["dt"] == b.summary()["dt"] and a.summary()["time"] == b.summary()["time"]
    for f in PROBE_VARS + ("k", "CP"):
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)


def _column_box(case, counts, want):
    """A box over all rows and the columns [a, b] whose nodes number exactly `want`."""
    H = 2 * case.ny * case.dy
    if want == 0:
        a = int(np.flatnonzero(counts == 0)[0])
        return ((a + 0.5) * case.dx, 0.0, 0.0, H)
    csum = np.concatenate([[0], np.cumsum(counts)])
    for a in range(len(counts)):
        b = int(np.searchsorted(csum, csum[a] + want))
        if b <= len(counts) and csum[b] - csum[a] == want:
            return ((a + 0.5) * case.dx, 0.0, (b - 1 - a) * case.dx, H)
    raise AssertionError("no column range holds %d nodes" % want)


def test_workgroup_edges(gpu, monkeypatch):
    """Lists of 0, 1, 64, 65, 256 and 257 nodes in one plan: list boundaries inside and at the edges of the
    256-lane workgroups of the node kernel."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = heat_keys(decks.step(700, 40, **BIG))   # (one node in each of 559 columns)
    a, b = gpu.Simulation(text, "gpu"), gpu.Simulation(text, "gpu")
    for s in (a, b):
        perturb(s, SEED)
    table = a.case.surface()
    counts = np.bincount(table["i"], minlength=a.case.nx)
    boxes = [_column_box(a.case, counts, n) for n in EDGES]
    a.record_surface(boxes=boxes, capacity=4)
    h = a.surface_history()
    np.testing.assert_array_equal(np.diff(h["box_off"]), EDGES)
    times, vals = make_twin(b, 3, boxes=boxes)
    a.step(3)
    h = a.surface_history()
    assert_history(h, times, vals, range(3))
    assert_stats(h, stats_oracle(times, vals, 0.0))
    assert_table(h, b.case.surface(boxes=boxes))
    assert (vals[1:, V["p"]] != vals[:-1, V["p"]]).any()


@pytest.mark.parametrize("name", list(LONG))
def test_several_workgroups(gpu, monkeypatch, name):
    """More nodes than one workgroup's 256 lanes and more needed cells than that, on every kind of the cell kernel."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    path = LONG[name][1]
    a = _make(gpu, name, False)
    a.record_surface(capacity=8)
    a.step(5)
    h = a.surface_history()
    times, vals = _twin(name, 5)
    assert_history(h, times, vals, range(5), name)
    assert_stats(h, stats_oracle(times, vals, 0.0), name)
    _assert_not_constant(name, vals, 5)
    assert len(h["i"]) > 256   # (every node is a needed cell of its own)
    sv = a.solver
    assert (dict(sv.lean_tile_last)["nt"] > 0) == (path == "tile")
    assert (sv.lns_steps > 0) == (path in ("sgl", "sgt")) and (sv.lnm_steps > 0) == (path == "mech")
    if path in ("sgl", "sgt"):
        assert sv.sk_mode == (1 if path == "sgl" else 2), sv.sk_mode


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_every_third_step_in_graphs(gpu, monkeypatch, name):
    """every=3 across the 26-step call, then arming after cached windows: exactly the twin's sampled rows."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    times, vals = _twin(name)
    a = _make(gpu, name, True)
    a.record_surface(every=3, capacity=64, weight="step")
    for n, res in GRAPH_SCHEDULE:
        a.step(n, residual=res)
    assert a.solver.graph_launches > 1
    h = a.surface_history()
    assert h["total"] == 13 and h["samples"] == 13
    assert_history(h, times, vals, range(2, 40, 3), name)
    assert_stats(h, stats_oracle(times, vals, 0.0, hi=40, every=3, weight="step"), name)
    # 26 steps unarmed, arm, 26 more: the windows cached before arming must not replay
    n = 26
    b = _make(gpu, name, True)
    b.step(n)
    before = b.solver.graph_launches
    assert before > 1
    b.record_surface(every=3, capacity=64)
    b.step(n)
    h = b.surface_history()
    assert len(times) == 52 and h["total"] == 8
    assert_history(h, times, vals, range(n + 2, 2 * n, 3), name)
    assert_stats(h, stats_oracle(times, vals, times[n - 1], lo=n, hi=2 * n, every=3), name)
    assert b.solver.graph_launches > before + 1   # captured again with the recorder, then replayed


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_ring_wraps_across_a_graph_call(gpu, monkeypatch, name):
    """Capacity 7 across the 26-step call (three graph windows): the last 7 rows, in order; then
    statistics alone, and a cleared recorder."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    times, vals = _twin(name)
    a, b = _make(gpu, name, True), _make(gpu, name, True)
    a.record_surface(capacity=7)
    b.record_surface(capacity=0)
    for n, res in GRAPH_SCHEDULE:
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.surface_history()
    assert a.solver.graph_launches > 1 and h["total"] == nsteps
    assert_history(h, times, vals, range(nsteps - 7, nsteps), name)
    want = stats_oracle(times, vals, 0.0, hi=nsteps)
    assert_stats(h, want, name)
    hb = b.surface_history()
    assert hb["total"] == nsteps and hb["values"].shape == (0, 10, vals.shape[2]) and hb["times"].shape == (0,)
    assert_stats(hb, want, name)
    a.clear_surface()
    z = a.surface_history()
    assert z["total"] == 0 and z["samples"] == 0 and not z["mean"].any() and z["values"].shape[0] == 0
    a.step(12)
    h = a.surface_history()
    assert_history(h, times, vals, range(nsteps + 5, nsteps + 12), name)
    assert_stats(h, stats_oracle(times, vals, times[nsteps - 1], lo=nsteps, hi=nsteps + 12), name)


def test_refusals_and_upload_mid_run(gpu, monkeypatch):
    """A lean N-S deck with isTurbulenceReset = 0 refuses before TurbStartIter, one strip of several
    refuses, and both are left without a recorder.  Refused re-arms leave the armed recorder as it was;
    an upload() rebuilds the plan, and the rows after it are those of a download."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = heat_keys(decks.step(37, 23, **BIG))
    late = text
    for k, v in (("isTurbulenceReset", 0), ("TurbStartIter", 1000)):
        late = decks.set_key(late, k, v)
    r = gpu.Simulation(late, "gpu")
    perturb(r, SEED)
    assert r.solver.lns_ok, r.solver.lns_why
    with pytest.raises(RuntimeError, match="TurbStartIter"):
        r.record_surface()
    with pytest.raises(RuntimeError):
        r.surface_history()   # the refused call left no recorder behind
    for lo, hi in ((0, 20), (20, 37)):   # a virtual rank's solver: one strip of two
        strip = gpu.Simulation(text, "gpu", gi0=lo, gi1=hi)
        with pytest.raises(RuntimeError, match="strip"):
            strip.record_surface()
    a = _make(gpu, "step_sgl", False)
    boxes, _ = targets(a.case)
    a.record_surface(boxes=boxes, capacity=8)
    a.step(6)
    assert a.solver.lns_steps > 0
    before = a.surface_history()
    flows = a.case.wall_heat_keys["flows"]
    for kw in (dict(cp_flow=flows + 1), dict(every=0), dict(boxes=boxes * 6), dict(boxes=[(0.0, 0.0, float("nan"), 1.0)]),
               dict(capacity=-1), dict(capacity=0, statistics=False), dict(boxes=boxes, capacity=2 ** 31 // (10 * len(before["i"])) + 1),
               dict(weight="mass")):
        with pytest.raises(ValueError):
            a.record_surface(**kw)
    after = a.surface_history()
    assert before.keys() == after.keys()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    perturb(a, SEED + 1)   # (set_records + upload: the plan is rebuilt)
    for k in range(2):   # (four steps: the last ones are lean N-S steps again)
        lean = a.solver.lns_steps
        a.step(4)
        h = a.surface_history()
        assert a.solver.lns_steps > lean
        a.solver.download()
        assert h["total"] == 6 + 4 * (k + 1)
        s = a.case.surface(boxes=boxes)
        np.testing.assert_array_equal(h["values"][-1], s["values"])
        np.testing.assert_array_equal(np.signbit(h["values"][-1]), np.signbit(s["values"]))
    assert_table(h, s)
    # arming again and again takes no new device arrays once they fit: the history stays exact
    for _ in range(3):
        a.record_surface(capacity=4)
    a.step(1)
    h = a.surface_history()
    a.solver.download()
    assert h["total"] == 1
    np.testing.assert_array_equal(h["values"][-1], a.case.surface()["values"])


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_all_observers_at_once(gpu, monkeypatch, name):
    """Probes, averaging, loads, wall heat and the surface armed together: each result is its result alone."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    sims = [_make(gpu, name, True) for _ in range(5)]
    all5, probes, avg, loads, heat = sims
    cells, _ = _cells(gpu, all5, name)
    boxes, cuts = targets(all5.case)
    all5.record_probes(cells, capacity=64)
    all5.start_averaging()
    all5.record_loads(boxes, cuts, capacity=64)
    all5.record_wall_heat(capacity=64)
    all5.record_surface(capacity=64)
    probes.record_probes(cells, capacity=64)
    avg.start_averaging()
    loads.record_loads(boxes, cuts, capacity=64)
    heat.record_wall_heat(capacity=64)
    for n, res in GRAPH_SCHEDULE:
        for s in sims:
            s.step(n, residual=res)
    times, vals = _twin(name)
    h = all5.surface_history()
    assert h["total"] == nsteps
    assert_history(h, times, vals, range(nsteps), name)
    assert_stats(h, stats_oracle(times, vals, 0.0, hi=nsteps), name)
    hp, hq = all5.probe_history(), probes.probe_history()
    np.testing.assert_array_equal(hp["values"], hq["values"])
    np.testing.assert_array_equal(hp["times"], hq["times"])
    np.testing.assert_array_equal(hp["times"], h["times"])
    A, B = all5.averages(), avg.averages()
    assert A["samples"] == B["samples"] == nsteps and A["time"] == B["time"]
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(A[k], B[k], err_msg=k)
    la, lb = all5.load_history(), loads.load_history()
    for k in ("times", "forces", "mass_flow"):
        np.testing.assert_array_equal(la[k], lb[k], err_msg=k)
    wa, wb = all5.wall_heat_history(), heat.wall_heat_history()
    for k in wa:
        np.testing.assert_array_equal(wa[k], wb[k], err_msg=k)
    assert all5.solver.graph_launches > 1
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(all5.solver, k) == getattr(probes.solver, k), k


def test_gpu_recorder_equals_the_cpu_recorder(gpu, monkeypatch):
    """The generic wedge: the CPU backend's recorder, row for row and bit for bit."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    name = "wedge_generic"
    g, c = _make(gpu, name, False), _make(gpu, name, False, backend="cpu")
    for s in (g, c):
        s.record_surface(capacity=64, every=2)
        for n, res in SCHEDULE:
            s.step(n, residual=res)
    hg, hc = g.surface_history(), c.surface_history()
    assert hg.keys() == hc.keys() and hg["total"] == 7 and len(hg["i"]) > 0
    for k in hg:
        np.testing.assert_array_equal(hg[k], hc[k], err_msg=k)
    np.testing.assert_array_equal(np.signbit(hg["values"]), np.signbit(hc["values"]))
