"""Per-step wall heat recorder on the device (hf2d_wallq_tick / hf2d_wallq_cells /
hf2d_wallq_fold, hip/wall_heat.hpp): the HeatFlux-X and HeatFlux-Y profiles and
their running statistics, written by up to three launches at the end of every
step from whichever representation is authoritative -- generic record, lean
inviscid arrays, lean N-S levels (SGL / SGT), lean mechanism state.

The oracle is a twin simulation of the same backend and settings without a
recorder, advanced with step(1) and a download after every step, and read
through Case.heat_flux_x / heat_flux_y (computed once per deck, shared, never
modified); the statistics' oracle is the rule transcribed in NumPy
(tests.test_wall_heat.stats_oracle) over the twin's profiles and times.  Every
comparison with the twin is bitwise.  The decks, paths and schedules are those
of test_gpu_probe_history.py with the heat-flux keys set; all runs start from
tests.perturb.perturb.  Each case asserts through the solver's counters that the
kernel it names ran, and that recording changed neither the counters nor the
final fields."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.model_families import REL
from tests.perturb import SCHEDULE, perturb
from tests.test_gpu_probe_history import BIG, DECKS, GRAPH_SCHEDULE, SEED, _assert_path, _cells, _tile
from tests.test_load_history import targets
from tests.test_wall_heat import assert_history, assert_stats, heat_keys, make_twin, node_counts, stats_oracle

pytestmark = pytest.mark.gpu

INVISCID = ("wedge_tile", "wedge_flat", "triple_point", "wedge_generic")
# decks whose lists and needed cells span several workgroups of 256 lanes, one per kind of the cell kernel
LONG = {
    "wedge_long": (lambda: decks.wedge15(800, 270, **BIG), "tile"),
    "step_long": (lambda: decks.step(700, 40, **BIG), "sgl"),
    "resonator_long": (lambda: decks.resonator(700, 40, **BIG), "sgt"),
    "scramjet_long": (lambda: decks.scramjet(700, 40, **BIG), "mech"),
}


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
    """times [n], x [n, 4, nx], y [n, ny] of the recorder-free twin after each of its one-step calls."""
    import openhyperflow2d_amd as hf

    return make_twin(_make(hf, name, False), nsteps)


def _assert_not_constant(name, twin, n):
    """A comparison of constants proves nothing: Q, Cp, St and the Y profile of the twin vary."""
    _, x, y = twin
    if name == "triple_point":   # no node: every profile is +0.0
        assert not x.any() and not y.any() and not np.signbit(x).any() and not np.signbit(y).any()
        return
    for v in (0, 2, 3):
        assert (x[1:n, v] != x[:n - 1, v]).any(), (name, v)
    assert (y[1:n] != y[:n - 1]).any(), name


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_history_equals_the_twin(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _make(gpu, name, graphs), _make(gpu, name, graphs)
    a.record_wall_heat(capacity=64)
    for n, res in sched:
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.wall_heat_history()
    times, x, y = twin = _twin(name)
    assert h["total"] == nsteps
    assert_history(h, times, x, y, range(nsteps), name)
    assert_stats(h, stats_oracle(times, x, y, 0.0, hi=nsteps), name)
    _assert_not_constant(name, twin, nsteps)
    xn, yn = node_counts(a.case)
    np.testing.assert_array_equal(h["x_nodes"], xn)
    np.testing.assert_array_equal(h["y_nodes"], yn)
    assert (xn.sum() > 0) == (name != "triple_point")
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


@pytest.mark.parametrize("name", list(LONG))
def test_several_workgroups(gpu, monkeypatch, name):
    """More lists than one workgroup's 256 lanes and more needed cells than that, on every kind of the cell kernel."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    path = LONG[name][1]
    a = _make(gpu, name, False)
    a.record_wall_heat(capacity=8)
    a.step(5)
    h = a.wall_heat_history()
    times, x, y = twin = _twin(name, 5)
    assert_history(h, times, x, y, range(5), name)
    assert_stats(h, stats_oracle(times, x, y, 0.0), name)
    _assert_not_constant(name, twin, 5)
    assert a.case.nx + a.case.ny > 256
    # (every node is a needed cell of its own, so the nodes bound the needed cells from below)
    assert max(h["x_nodes"].sum(), h["y_nodes"].sum()) > 256
    sv = a.solver
    assert (dict(sv.lean_tile_last)["nt"] > 0) == (path == "tile")
    assert (sv.lns_steps > 0) == (path in ("sgl", "sgt")) and (sv.lnm_steps > 0) == (path == "mech")
    if path in ("sgl", "sgt"):
        assert sv.sk_mode == (1 if path == "sgl" else 2), sv.sk_mode


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_every_third_step_in_graphs(gpu, monkeypatch, name):
    """every=3 across the 26-step call, then arming after cached windows: exactly the twin's sampled rows."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    times, x, y = _twin(name)
    a = _make(gpu, name, True)
    a.record_wall_heat(every=3, capacity=64, weight="step")
    for n, res in GRAPH_SCHEDULE:
        a.step(n, residual=res)
    assert a.solver.graph_launches > 1
    h = a.wall_heat_history()
    assert h["total"] == 13 and h["samples"] == 13
    assert_history(h, times, x, y, range(2, 40, 3), name)
    assert_stats(h, stats_oracle(times, x, y, 0.0, hi=40, every=3, weight="step"), name)
    # 26 steps unarmed, arm, 26 more: the windows cached before arming must not replay
    n = 26
    b = _make(gpu, name, True)
    b.step(n)
    before = b.solver.graph_launches
    assert before > 1
    b.record_wall_heat(every=3, capacity=64)
    b.step(n)
    h = b.wall_heat_history()
    assert len(times) == 52 and h["total"] == 8
    assert_history(h, times, x, y, range(n + 2, 2 * n, 3), name)
    assert_stats(h, stats_oracle(times, x, y, times[n - 1], lo=n, hi=2 * n, every=3), name)
    assert b.solver.graph_launches > before + 1   # captured again with the recorder, then replayed


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_ring_wraps_across_a_graph_call(gpu, monkeypatch, name):
    """Capacity 7 across the 26-step call (three graph windows): the last 7 rows, in order; then
    statistics alone, and a cleared recorder."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    times, x, y = _twin(name)
    a, b = _make(gpu, name, True), _make(gpu, name, True)
    a.record_wall_heat(capacity=7)
    b.record_wall_heat(capacity=0)
    for n, res in GRAPH_SCHEDULE:
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.wall_heat_history()
    assert a.solver.graph_launches > 1 and h["total"] == nsteps
    assert_history(h, times, x, y, range(nsteps - 7, nsteps), name)
    want = stats_oracle(times, x, y, 0.0, hi=nsteps)
    assert_stats(h, want, name)
    hb = b.wall_heat_history()
    assert hb["total"] == nsteps and hb["x"].shape == (0, 4, b.case.nx) and hb["times"].shape == (0,)
    assert_stats(hb, want, name)
    a.clear_wall_heat()
    z = a.wall_heat_history()
    assert z["total"] == 0 and z["samples"] == 0 and not z["mean_x"].any() and z["x"].shape[0] == 0
    a.step(12)
    h = a.wall_heat_history()
    assert_history(h, times, x, y, range(nsteps + 5, nsteps + 12), name)
    assert_stats(h, stats_oracle(times, x, y, times[nsteps - 1], lo=nsteps, hi=nsteps + 12), name)


def test_a_refused_rearm_leaves_the_recorder_whole(gpu, monkeypatch):
    """A lean N-S deck with isTurbulenceReset = 0 refuses before TurbStartIter and is left without a
    recorder.  With the Y profile armed, refused re-arms leave the armed recorder as it was, also
    after an upload() that rebuilds the plan."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = heat_keys(decks.step(37, 23, **BIG))
    late = text
    for k, v in (("isTurbulenceReset", 0), ("TurbStartIter", 1000)):
        late = decks.set_key(late, k, v)
    r = gpu.Simulation(late, "gpu")
    perturb(r, SEED)
    assert r.solver.lns_ok, r.solver.lns_why
    with pytest.raises(RuntimeError, match="TurbStartIter"):
        r.record_wall_heat()
    with pytest.raises(RuntimeError):
        r.wall_heat_history()   # the refused call left no recorder behind
    a = gpu.Simulation(text, "gpu")
    perturb(a, SEED)
    a.record_wall_heat(x=False, capacity=8)
    a.step(3)
    before = a.wall_heat_history()
    with pytest.raises(ValueError):
        a.record_wall_heat(cp_flow=a.case.wall_heat_keys["flows"] + 1)
    with pytest.raises(ValueError):
        a.record_wall_heat(every=0)
    after = a.wall_heat_history()
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    perturb(a, SEED + 1)   # (set_records + upload: the plan is rebuilt)
    a.step(2)
    h = a.wall_heat_history()
    a.solver.download()
    assert h["total"] == 5 and not h["x"].any() and not h["x_nodes"].any()
    np.testing.assert_array_equal(h["y"][-1], a.case.heat_flux_y())
    # arming again and again takes no new device arrays once they fit: the history stays exact
    for _ in range(3):
        a.record_wall_heat(capacity=4)
    a.step(1)
    h = a.wall_heat_history()
    a.solver.download()
    assert h["total"] == 1
    np.testing.assert_array_equal(h["x"][-1], a.case.heat_flux_x())
    np.testing.assert_array_equal(h["y"][-1], a.case.heat_flux_y())


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_all_observers_at_once(gpu, monkeypatch, name):
    """Probes, averaging, loads and wall heat armed together: each result is its result alone."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    sims = [_make(gpu, name, True) for _ in range(4)]
    all4, probes, avg, loads = sims
    cells, _ = _cells(gpu, all4, name)
    boxes, cuts = targets(all4.case)
    all4.record_probes(cells, capacity=64)
    all4.start_averaging()
    all4.record_loads(boxes, cuts, capacity=64)
    all4.record_wall_heat(capacity=64)
    probes.record_probes(cells, capacity=64)
    avg.start_averaging()
    loads.record_loads(boxes, cuts, capacity=64)
    for n, res in GRAPH_SCHEDULE:
        for s in sims:
            s.step(n, residual=res)
    times, x, y = _twin(name)
    h = all4.wall_heat_history()
    assert h["total"] == nsteps
    assert_history(h, times, x, y, range(nsteps), name)
    assert_stats(h, stats_oracle(times, x, y, 0.0, hi=nsteps), name)
    hp, hq = all4.probe_history(), probes.probe_history()
    np.testing.assert_array_equal(hp["values"], hq["values"])
    np.testing.assert_array_equal(hp["times"], hq["times"])
    np.testing.assert_array_equal(hp["times"], h["times"])
    A, B = all4.averages(), avg.averages()
    assert A["samples"] == B["samples"] == nsteps and A["time"] == B["time"]
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(A[k], B[k], err_msg=k)
    la, lb = all4.load_history(), loads.load_history()
    for k in ("times", "forces", "mass_flow"):
        np.testing.assert_array_equal(la[k], lb[k], err_msg=k)
    assert all4.solver.graph_launches > 1
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(all4.solver, k) == getattr(probes.solver, k), k


@pytest.mark.parametrize("name", list(DECKS))
def test_gpu_against_cpu(gpu, monkeypatch, name):
    """The CPU backend's history of the same deck: bitwise on the inviscid
    decks; on the viscous ones every series agrees to the project's GPU / CPU
    bound, max |diff| <= 1e-9 * max |value| (tests/model_families.py)."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    c = _make(gpu, name, False, backend="cpu")
    c.record_wall_heat(capacity=64)
    nsteps = sum(n for n, _ in SCHEDULE)
    for n, res in SCHEDULE:
        c.step(n, residual=res)
    h = c.wall_heat_history()
    _, x, y = _twin(name)
    xn, yn = node_counts(c.case)
    np.testing.assert_array_equal(h["x_nodes"], xn)
    np.testing.assert_array_equal(h["y_nodes"], yn)
    series = [(v, x[:nsteps, k], h["x"][:, k]) for k, v in enumerate(("Q", "Alpha", "Cp", "St"))]
    series.append(("Y", y[:nsteps], h["y"]))
    for what, g, cpu in series:
        if name in INVISCID:
            np.testing.assert_array_equal(g, cpu, err_msg=what)
        else:
            d, top = np.abs(g - cpu).max(), np.abs(cpu).max()
            print("%s %s: max |diff| %.3e, max |value| %.6e" % (name, what, d, top))
            assert d <= REL * top, (what, d, top)
