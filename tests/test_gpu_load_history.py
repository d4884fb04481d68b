"""Per-step load recorder on the device (hf2d_loads_terms / hf2d_loads_fold,
hip/load_history.hpp): the pressure and friction parts of the body force of
every box and the mass flow through every x cut, written by two launches at the
end of every step from whichever representation is authoritative -- generic
record, lean inviscid arrays, lean N-S levels (SGL / SGT), lean mechanism state.

The oracle is a twin simulation of the same backend and settings without a
recorder, advanced with step(1) and a download after every step, and read
through Case.force_parts and Case.mass_flow_x (computed once per deck, shared,
never modified); every comparison is bitwise.  The decks, paths and schedules
are those of test_gpu_probe_history.py; all runs start from
tests.perturb.perturb.  Each case asserts through the solver's counters that
the kernel it names ran, and that recording changed neither the counters nor
the final fields."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.model_families import REL
from tests.perturb import SCHEDULE, perturb
from tests.test_gpu_probe_history import BIG, DECKS, GRAPH_SCHEDULE, SEED, _assert_path, _cells, _sim, _tile
from tests.test_load_history import cut_counts, host_loads
from tests.test_load_history import targets as base_targets

pytestmark = pytest.mark.gpu

INVISCID = ("wedge_tile", "wedge_flat", "triple_point", "wedge_generic")
# The fold stages a list in blocks of 256 terms (LOADS_FOLD_STAGE) and adds them in groups of 32
# (LOADS_FOLD_GROUP).  Decks for the fold alone, one per kind of the term kernel: their longest
# lists fill a block and go on (351: one full block and a tail; 559 .. 748: two and a tail), and end
# inside a group.  wedge15(200, 40), the issue's fallback, has lists of 96 and 100 terms: more than
# one wavefront of 64 lanes, inside one block.
STAGE, GROUP = 256, 32
LONG = {
    "wedge_100": (lambda: decks.wedge15(200, 40, **BIG), "tile", False),
    "wedge_long": (lambda: decks.wedge15(800, 270, **BIG), "tile", True),
    "step_long": (lambda: decks.step(700, 40, **BIG), "sgl", True),
    "resonator_long": (lambda: decks.resonator(700, 40, **BIG), "sgt", True),
    "scramjet_long": (lambda: decks.scramjet(700, 40, **BIG), "mech", True),
}


def targets(case):
    """The issue's three boxes and five cuts, and a sixth cut of one cell (a list of one term)."""
    boxes, cuts = base_targets(case)
    solid = np.asarray(case.field("solid"))
    im = case.nx // 2
    j = int(np.flatnonzero(solid[im] == 0.0)[-1])
    return boxes, cuts + [((im + 0.5) * case.dx, (j + 0.25) * case.dy, case.dy)]


def _make(gpu, name, graphs):
    if name in DECKS:
        return _sim(gpu, name, graphs)
    s = gpu.Simulation(LONG[name][0](), "gpu")
    perturb(s, SEED)
    s.solver.use_graph = graphs
    return s


@functools.lru_cache(maxsize=None)
def _twin(name, nsteps=52):
    """times [n], forces [n, nboxes, 4], mass_flow [n, ncuts], term counts and
    spans of the recorder-free twin after each of its one-step calls."""
    import openhyperflow2d_amd as hf

    s = _make(hf, name, False)
    boxes, cuts = targets(s.case)
    times, forces, flows = [], [], []
    for _ in range(nsteps):
        s.step(1)
        s.solver.download()
        f, counts, span, totals, mf = host_loads(s.case, boxes, cuts)
        np.testing.assert_array_equal(f[:, 0] + f[:, 1], totals[:, 0])   # (force_parts against x_force / y_force)
        np.testing.assert_array_equal(f[:, 2] + f[:, 3], totals[:, 1])
        forces.append(f)
        flows.append(mf)
        times.append(s.summary()["time"])
    out = (np.array(times), np.array(forces), np.array(flows), counts, span, cut_counts(s.case, cuts))
    for a in out:
        a.setflags(write=False)
    return out


def _assert_rows(h, twin, lo, hi):
    times, forces, flows, counts, span, ccounts = twin
    assert h["forces"].shape == (hi - lo,) + forces.shape[1:] and h["mass_flow"].shape == (hi - lo, flows.shape[1])
    for b in range(forces.shape[1]):
        for q in range(4):
            np.testing.assert_array_equal(h["forces"][:, b, q], forces[lo:hi, b, q], err_msg="box %d part %d" % (b, q))
    for c in range(flows.shape[1]):
        np.testing.assert_array_equal(h["mass_flow"][:, c], flows[lo:hi, c], err_msg="cut %d" % c)
    np.testing.assert_array_equal(h["times"], times[lo:hi])
    np.testing.assert_array_equal(h["terms"]["box_terms"], counts)
    np.testing.assert_array_equal(h["terms"]["cut_terms"], ccounts)
    np.testing.assert_array_equal(h["span"], span)


def _assert_not_constant(name, twin, n):
    """A comparison of constants proves nothing: some force list and some cut of the twin vary."""
    _, forces, flows, counts, _, _ = twin
    assert any(len(set(flows[:n, c].tolist())) > 1 for c in range(flows.shape[1])), name
    if counts.sum() > 0:
        assert any(len(set(forces[:n, b, q].tolist())) > 1 for b in range(forces.shape[1]) for q in range(4)), name
    else:
        assert name == "triple_point" and (forces == 0).all() and not np.signbit(forces).any()


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_history_equals_the_twin(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _sim(gpu, name, graphs), _sim(gpu, name, graphs)
    boxes, cuts = targets(a.case)
    a.record_loads(boxes, cuts, capacity=64)
    for n, res in sched:
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.load_history()
    twin = _twin(name)
    assert h["total"] == nsteps
    _assert_rows(h, twin, 0, nsteps)
    _assert_not_constant(name, twin, nsteps)
    ct = h["terms"]["cut_terms"]
    assert ct[4] == 0 and ct[5] == 1 and (h["terms"]["box_terms"][2] == 0).all()   # lists of 0 terms and of 1 term
    assert (h["mass_flow"][:, 4] == 0).all() and not np.signbit(h["mass_flow"][:, 4]).any()
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
def test_fold_of_long_lists(gpu, monkeypatch, name):
    """Lists that span several of the fold's 256-term blocks, on every kind of the term kernel; and
    wedge15(200, 40): lists of more than 64 terms that are no multiple of 64."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    _, path, blocks = LONG[name]
    a = _make(gpu, name, False)
    boxes, cuts = targets(a.case)
    a.record_loads(boxes, cuts, capacity=8)
    a.step(5)
    h = a.load_history()
    twin = _twin(name, 5)
    _assert_rows(h, twin, 0, 5)
    _assert_not_constant(name, twin, 5)
    lens = h["terms"]["box_terms"].ravel().tolist() + h["terms"]["cut_terms"].tolist()
    assert 0 in lens and 1 in lens, lens
    if blocks:
        assert any(STAGE < n < 2 * STAGE and n % GROUP for n in lens), lens       # a full block and a tail
        assert any(n > 2 * STAGE and n % STAGE and n % GROUP for n in lens), lens   # two full blocks and a tail
    else:
        assert any(n > 64 and n % 64 for n in lens), lens
    sv = a.solver
    assert (dict(sv.lean_tile_last)["nt"] > 0) == (path == "tile")
    assert (sv.lns_steps > 0) == (path in ("sgl", "sgt")) and (sv.lnm_steps > 0) == (path == "mech")
    if path in ("sgl", "sgt"):
        assert sv.sk_mode == (1 if path == "sgl" else 2), sv.sk_mode


def test_a_refused_rearm_leaves_the_recorder_whole(gpu, monkeypatch):
    """Cuts armed; a re-arm with boxes is refused (wall terms on a lean N-S deck before TurbStartIter).
    The armed lists and the ring's shape stay, also after an upload() that rebuilds the plan."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.step(37, 23, **BIG)
    for k, v in (("isTurbulenceReset", 0), ("TurbStartIter", 1000)):
        text = decks.set_key(text, k, v)
    a = gpu.Simulation(text, "gpu")
    perturb(a, SEED)
    assert a.solver.lns_ok, a.solver.lns_why
    boxes, cuts = targets(a.case)
    a.record_loads((), cuts[:2], capacity=8)
    a.step(3)
    with pytest.raises(RuntimeError, match="TurbStartIter"):
        a.record_loads(boxes, cuts, capacity=8)
    with pytest.raises(ValueError):
        a.record_loads(boxes, cuts, capacity=0)
    perturb(a, SEED + 1)   # (set_records + upload: the plan is rebuilt)
    a.step(2)
    h = a.load_history()
    assert h["total"] == 5 and h["forces"].shape == (5, 0, 4) and h["mass_flow"].shape == (5, 2)
    a.solver.download()
    np.testing.assert_array_equal(h["mass_flow"][-1], [a.case.mass_flow_x(*c) for c in cuts[:2]])
    np.testing.assert_array_equal(h["terms"]["cut_terms"], cut_counts(a.case, cuts[:2]))
    # arming again and again takes no new device arrays once they fit: the history stays exact
    for _ in range(3):
        a.record_loads((), cuts[:3], capacity=4)
    a.step(1)
    a.solver.download()
    h = a.load_history()
    assert h["total"] == 1 and h["mass_flow"].shape == (1, 3)
    np.testing.assert_array_equal(h["mass_flow"][-1], [a.case.mass_flow_x(*c) for c in cuts[:3]])


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_ring_wraps_across_a_graph_call(gpu, monkeypatch, name):
    """Capacity 7 across the 26-step call (three graph windows): the last 7 rows, in order."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    a = _sim(gpu, name, True)
    boxes, cuts = targets(a.case)
    a.record_loads(boxes, cuts, capacity=7)
    for n, res in GRAPH_SCHEDULE:
        a.step(n, residual=res)
    h = a.load_history()
    assert a.solver.graph_launches > 1
    assert h["total"] == nsteps
    _assert_rows(h, _twin(name), nsteps - 7, nsteps)


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_arming_after_cached_windows(gpu, monkeypatch, name):
    """26 steps, arm, 26 more: exactly 26 rows, the twin's steps 27 .. 52.  The
    windows cached and replayed before arming hold no recorder launch and must
    not replay (the arming generation in mode_signature); nor may those of the
    first ring after arming again."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    n = 26
    a = _sim(gpu, name, True)
    boxes, cuts = targets(a.case)
    a.step(n)
    before = a.solver.graph_launches
    assert before > 1
    a.record_loads(boxes, cuts, capacity=64)
    a.step(n)
    h = a.load_history()
    twin = _twin(name)
    assert len(twin[0]) == 52 and h["total"] == n
    _assert_rows(h, twin, n, 2 * n)
    assert a.solver.graph_launches > before + 1   # captured again with the recorder, then replayed
    a.record_loads(boxes[:1], cuts[:2], capacity=64)
    a.step(n)
    h = a.load_history()
    assert h["total"] == n and h["forces"].shape == (n, 1, 4) and h["mass_flow"].shape == (n, 2)
    # (only the count and the ring are checked here: the twin ends at step 52)
    assert np.isfinite(h["forces"]).all() and (np.diff(h["times"]) > 0).all() and h["times"][0] > twin[0][-1]


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_three_observers_at_once(gpu, monkeypatch, name):
    """Probes, averaging and loads armed together: each result is its result alone."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    sims = [_sim(gpu, name, True) for _ in range(3)]
    all3, probes, avg = sims
    cells, _ = _cells(gpu, all3, name)
    boxes, cuts = targets(all3.case)
    all3.record_probes(cells, capacity=64)
    all3.start_averaging()
    all3.record_loads(boxes, cuts, capacity=64)
    probes.record_probes(cells, capacity=64)
    avg.start_averaging()
    for n, res in GRAPH_SCHEDULE:
        for s in sims:
            s.step(n, residual=res)
    h = all3.load_history()
    assert h["total"] == nsteps
    _assert_rows(h, _twin(name), 0, nsteps)
    hp, hq = all3.probe_history(), probes.probe_history()
    np.testing.assert_array_equal(hp["values"], hq["values"])
    np.testing.assert_array_equal(hp["times"], hq["times"])
    np.testing.assert_array_equal(hp["times"], h["times"])
    A, B = all3.averages(), avg.averages()
    assert A["samples"] == B["samples"] == nsteps and A["time"] == B["time"]
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(A[k], B[k], err_msg=k)
    assert all3.solver.graph_launches > 1
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(all3.solver, k) == getattr(probes.solver, k), k


@pytest.mark.parametrize("name", list(DECKS))
def test_gpu_against_cpu(gpu, monkeypatch, name):
    """The CPU backend's history of the same deck: bitwise on the inviscid
    decks; on the viscous ones every series agrees to the project's GPU / CPU
    bound, max |diff| <= 1e-9 * max |value| (tests/model_families.py)."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    gen, kw, _, _ = DECKS[name]
    c = gpu.Simulation(gen(), "cpu")
    perturb(c, SEED)
    boxes, cuts = targets(c.case)
    c.record_loads(boxes, cuts, capacity=64)
    nsteps = sum(n for n, _ in SCHEDULE)
    for n, res in SCHEDULE:
        c.step(n, residual=res)
    h = c.load_history()
    _, forces, flows, counts, span, ccounts = _twin(name)
    np.testing.assert_array_equal(h["terms"]["cut_terms"], ccounts)
    np.testing.assert_array_equal(h["terms"]["box_terms"], counts)
    np.testing.assert_array_equal(h["span"], span)
    series = [("box %d part %d" % (b, q), forces[:nsteps, b, q], h["forces"][:, b, q])
              for b in range(forces.shape[1]) for q in range(4)]
    series += [("cut %d" % q, flows[:nsteps, q], h["mass_flow"][:, q]) for q in range(flows.shape[1])]
    for what, g, cpu in series:
        if name in INVISCID:
            np.testing.assert_array_equal(g, cpu, err_msg=what)
        else:
            d, top = np.abs(g - cpu).max(), np.abs(cpu).max()
            print("%s %s: max |diff| %.3e, max |value| %.6e" % (name, what, d, top))
            assert d <= REL * top, (what, d, top)
