"""Per-step probe recorder on the device (hf2d_probe_record, hip/probe_history.hpp):
one row (p, T, rho, U, V) per probe and step, written by the last launch of
every step from whichever representation is authoritative -- generic record,
lean inviscid arrays, lean N-S levels (SGL / SGT), lean mechanism state.

The oracle is a twin simulation of the same backend and settings without a
recorder, advanced with step(1) and read with field() and summary()["time"]
after every step (computed once per deck, shared, never modified); every
comparison is bitwise.  All runs start from tests.perturb.perturb.  Each case
asserts through the solver's counters that the kernel it names ran, and that
recording changed neither the counters nor the final fields."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.perturb import SCHEDULE, perturb

pytestmark = pytest.mark.gpu

SEED = 1
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
GRAPH_SCHEDULE = SCHEDULE + [(26, False)]   # the schedule of the existing graph tests (a 26-step call fills windows)

# name -> (deck text, Simulation keywords, solver attributes, path the deck reaches)
DECKS = {
    "wedge_tile": (lambda: decks.wedge15(67, 23, **BIG), {}, {"lean_cpt": 1, "lean_tj": 16}, "tile"),
    "wedge_flat": (lambda: decks.wedge15(40, 7, **BIG), {}, {}, "flat"),
    "triple_point": (lambda: decks.triple_point(160, 51, **BIG), {}, {"lean_cpt": 1, "lean_tj": 16}, "tile3"),
    "step_sgl": (lambda: decks.step(37, 23, **BIG), {}, {"lean_tj": 16}, "sgl"),
    "resonator_sgt": (lambda: decks.resonator(37, 23, **BIG), {}, {"lean_tj": 16}, "sgt"),
    "scramjet_mech": (lambda: decks.scramjet(37, 23, **BIG), {}, {}, "mech"),
    "step_split": (lambda: decks.step(37, 23, **BIG), {}, {"lean_ns": False}, "split"),
    "wedge_generic": (lambda: decks.wedge15(67, 23, **BIG), {"lean": False}, {}, "generic"),
}


def _sim(gpu, name, graphs):
    gen, kw, attrs, _ = DECKS[name]
    s = gpu.Simulation(gen(), "gpu", **kw)
    perturb(s, SEED)
    for k, v in attrs.items():
        setattr(s.solver, k, v)
    s.solver.use_graph = graphs
    return s


@functools.lru_cache(maxsize=None)
def _twin(name, nsteps=52):
    """times [n] and fields {var: [n, nx, ny]} of the recorder-free twin after
    each of its one-step calls (52: the longest run of this file)."""
    import openhyperflow2d_amd as hf

    s = _sim(hf, name, False)
    times, fields = [], {v: [] for v in PROBE_VARS}
    for _ in range(nsteps):
        s.step(1)
        s.solver.download()
        for v in PROBE_VARS:
            fields[v].append(np.asarray(s.case.field(v)).copy())
        times.append(s.summary()["time"])
    out = {v: np.array(a) for v, a in fields.items()}
    for a in out.values():
        a.setflags(write=False)
    return np.array(times), out


def _rows(twin_fields, cells, lo, hi):
    return np.array([[[twin_fields[v][k][i, j] for v in PROBE_VARS] for i, j in cells] for k in range(lo, hi)])


def _tile(gpu, name, nx, ny):
    """(TI, TJ) of the deck's tile kernel (None: the path has no tiles)."""
    path = DECKS[name][3]
    if path in ("tile", "tile3", "sgl", "sgt", "split"):   # (lean_tj = 16: two tile rows on these low grids)
        T = gpu.native().lean_tile_geom(nx, ny, 256, 16, 1)
        return T["TI"], T["TJ"]
    if path == "mech":
        return 16, 16
    if path == "generic":
        return 16, 16   # no tiles: the same places as the lean runs of the deck
    return None


def _cells(gpu, sim, name):
    """Non-solid cells on the grid's four edges, on both sides of the first
    tile boundary in x and in y, and one interior cell."""
    solid = sim.field("solid")
    nx, ny = solid.shape
    im, jm = nx // 2, ny // 2
    want = [(im + 1, jm + 1)]
    for i in (0, nx - 1):   # the edges: the middle-most and the last non-solid cell of each (none: a solid edge)
        free = np.flatnonzero(solid[i] == 0.0)
        want += [(i, int(j)) for j in free[[len(free) // 2, -1]]] if len(free) else []
    for j in (0, ny - 1):
        free = np.flatnonzero(solid[:, j] == 0.0)
        want += [(int(i), j) for i in free[[len(free) // 2, -1]]] if len(free) else []
    T = _tile(gpu, name, nx, ny)
    if T is not None:
        TI, TJ = T
        assert 0 < TI < nx and 0 < TJ < ny, (T, nx, ny)   # more than one tile in both directions
        # both sides of the first tile boundary, where both are gas: the middle-most and the last such place
        rows = np.flatnonzero((solid[TI - 1] == 0.0) & (solid[TI] == 0.0))
        cols = np.flatnonzero((solid[:, TJ - 1] == 0.0) & (solid[:, TJ] == 0.0))
        assert len(rows) and len(cols), (name, T)
        for j in rows[[len(rows) // 2, -1]]:
            want += [(TI - 1, int(j)), (TI, int(j))]
        for i in cols[[len(cols) // 2, -1]]:
            want += [(int(i), TJ - 1), (int(i), TJ)]
    cells = [c for c in dict.fromkeys(want) if solid[c] == 0.0]
    edges = [any(c[0] == 0 for c in cells), any(c[0] == nx - 1 for c in cells), any(c[1] == 0 for c in cells),
             any(c[1] == ny - 1 for c in cells)]
    assert sum(edges) >= 3 and len(cells) >= 6, (cells, edges)   # (the scramjet's top row is solid)
    return cells, T


def _assert_path(sv, name, T):
    path = DECKS[name][3]
    last = dict(sv.lean_tile_last)
    if path in ("tile", "tile3"):
        assert last["nt"] == 256 and (last["TI"], last["TJ"]) == T, last
        assert last["nbi"] > 1 and last["nbj"] > 1, last
        assert sv.lean_sg_ok == (path == "tile")
    elif path == "flat":
        assert sv.lean_ok and last["nt"] == 0, last
    else:
        assert last["nt"] == 0, last
    assert (sv.lns_steps > 0) == (path in ("sgl", "sgt")), sv.lns_steps
    assert (sv.lnm_steps > 0) == (path == "mech"), sv.lnm_steps
    if path in ("sgl", "sgt"):
        assert sv.lns_ok, sv.lns_why
    if path == "split":
        assert sv.lns_ok and not sv.lean_ns   # eligible, switched off
    if path == "generic":
        assert not sv.lean


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_history_equals_the_twin(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _sim(gpu, name, graphs), _sim(gpu, name, graphs)
    cells, T = _cells(gpu, a, name)
    a.record_probes(cells, capacity=64)
    for n, res in sched:
        a.step(n, residual=res)
        b.step(n, residual=res)
    h = a.probe_history()
    times, fields = _twin(name)
    assert h["total"] == nsteps and h["values"].shape == (nsteps, len(cells), 5)
    assert h["owned"].all()
    want = _rows(fields, cells, 0, nsteps)
    for q, c in enumerate(cells):
        for v, var in enumerate(PROBE_VARS):
            np.testing.assert_array_equal(h["values"][:, q, v], want[:, q, v], err_msg="%s at %s" % (var, c))
    np.testing.assert_array_equal(h["times"], times[:nsteps])
    # the named kernel ran, and recording left neither the lean state nor the graphs
    for s in (a, b):
        _assert_path(s.solver, name, T)
    assert (a.solver.graph_launches > 1) == graphs, a.solver.graph_launches
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(a.solver, k) == getattr(b.solver, k), k
    # reading the history moved nothing: the next steps and the final fields are the plain run's
    assert a.summary()["dt"] == b.summary()["dt"] and a.summary()["time"] == b.summary()["time"]
    for f in PROBE_VARS + ("k", "CP"):
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_ring_wraps_across_a_graph_call(gpu, monkeypatch, name):
    """Capacity 7 across the 26-step call (three graph windows): the last 7 rows, in order."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    nsteps = sum(n for n, _ in GRAPH_SCHEDULE)
    a = _sim(gpu, name, True)
    cells, _ = _cells(gpu, a, name)
    a.record_probes(cells, capacity=7)
    for n, res in GRAPH_SCHEDULE:
        a.step(n, residual=res)
    h = a.probe_history()
    times, fields = _twin(name)
    assert a.solver.graph_launches > 1
    assert h["total"] == nsteps and h["values"].shape == (7, len(cells), 5)
    np.testing.assert_array_equal(h["values"], _rows(fields, cells, nsteps - 7, nsteps))
    np.testing.assert_array_equal(h["times"], times[nsteps - 7:nsteps])


@pytest.mark.parametrize("n", [12, 26])
@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_arming_after_cached_windows(gpu, monkeypatch, name, n):
    """n steps, arm, n more: exactly n rows, the twin's steps n + 1 .. 2 n.
    A window captured before arming has no recorder launch and must not replay
    (the arming generation in mode_signature).  n = 26: windows were cached
    and replayed before arming (a 12-step call ends before its second window
    is full, so it caches none)."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a = _sim(gpu, name, True)
    cells, _ = _cells(gpu, a, name)
    a.step(n)
    before = a.solver.graph_launches
    assert (before > 1) == (n == 26), before
    a.record_probes(cells, capacity=64)
    a.step(n)
    h = a.probe_history()
    times, fields = _twin(name)
    assert len(times) == 52
    assert h["total"] == n and h["values"].shape == (n, len(cells), 5)
    np.testing.assert_array_equal(h["values"], _rows(fields, cells, n, 2 * n))
    np.testing.assert_array_equal(h["times"], times[n:2 * n])
    if n == 26:
        assert a.solver.graph_launches > before + 1   # captured again with the recorder, then replayed
        # arming again: the windows of the first ring must not replay either
        a.record_probes(cells[:2], capacity=64)
        a.step(n)
        h = a.probe_history()
        assert h["total"] == n and h["values"].shape == (n, 2, 5)
        # (only the count and the ring are checked here: the twin ends at step 52)
        assert np.isfinite(h["values"]).all() and (np.diff(h["times"]) > 0).all()
        assert h["times"][0] > times[-1]


@pytest.mark.parametrize("p2p", [False, True], ids=["local", "p2p"])
@pytest.mark.parametrize("deck", ["wedge", "step"])
def test_strips_record_their_own_probes(gpu, monkeypatch, deck, p2p):
    """Three strips on virtual ranks, every solver armed with the same global
    probe list: each probe is owned by exactly one rank, and the owners' rows
    together are the one-GPU history."""
    from openhyperflow2d_amd.parallel.strips import balanced_columns
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(240, 60, **BIG) if deck == "wedge" else decks.step(240, 80, **BIG)
    ref = gpu.Simulation(text, "gpu")
    perturb(ref, SEED)
    solid = ref.field("solid")
    nx, ny = solid.shape
    parts = balanced_columns(solid, 3)
    want = []
    for a, b in parts:   # first and last owned column of every strip, and an interior cell
        for i in (a, b - 1, (a + b) // 2):
            free = np.flatnonzero(solid[i] == 0.0)
            want += [(int(i), int(free[len(free) // 2])), (int(i), int(free[0])), (int(i), int(free[-1]))]
    cells = list(dict.fromkeys(want))
    assert len(cells) <= 64
    ref.record_probes(cells, capacity=32)
    for n, res in SCHEDULE:
        ref.step(n, residual=res)
    one = ref.probe_history()
    held, stats = [], {}

    def setup(s):
        held.append(s)
        s.record_probes(cells, 32)

    _virtual_ranks(gpu, text, 3, SCHEDULE, lean=True, p2p=p2p, setup=setup, parts=parts,
                   case_hook=lambda c: perturb(c, SEED), stats=stats)
    if deck == "step":
        assert min(stats["lns_steps"]) > 0 and ref.solver.lns_steps > 0, stats
    hist = [dict(s.probe_history()) for s in held]
    owned = np.array([np.asarray(h["owned"]) for h in hist])
    assert (owned.sum(axis=0) == 1).all(), owned
    for r, (a, b) in enumerate(parts):
        assert owned[r].tolist() == [a <= i < b for i, _ in cells]
    got = np.zeros_like(one["values"])
    for h, o in zip(hist, owned):
        assert int(h["total"]) == one["total"] == 14
        v = np.asarray(h["values"])
        assert (v[:, ~o] == 0).all()
        got[:, o] = v[:, o]
        np.testing.assert_array_equal(np.asarray(h["times"]), one["times"])
    np.testing.assert_array_equal(got, one["values"])
