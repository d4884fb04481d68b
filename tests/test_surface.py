"""Per-node wall surface distributions: the oracle Case.surface and the per-step
recorder Simulation.record_surface / surface_history on the CPU backend, which
evaluates the shared plan (core/surface_plan.hpp) on its own arrays after every
step.

The oracle is pinned to the pieces it unfolds: its p to field("p"), its signed
areas times p, folded in list order, to Case.force_parts bit for bit, its q_y /
q_x folded with the max-or-first rule to Case.heat_flux_x / heat_flux_y bit for
bit, and its friction terms to the friction folds within the rounding of the
two associations.  The recorder's oracle is a twin simulation without a
recorder, advanced with step(1), downloaded after every step and read through
Case.surface and summary()["time"] (computed once per deck, shared, never
modified); the statistics' oracle is the update rule transcribed in NumPy over
the twin's values and times.  Every comparison with the twin is bitwise.  All
runs start from tests.perturb.perturb."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import SURFACE_VARS
from tests.perturb import RECORD, perturb
from tests.test_load_history import empty_box, targets
from tests.test_wall_heat import BIG, CT_OFFSET, KEYS, SEED, _py, heat_keys

NSTEPS = 12
V = {name: k for k, name in enumerate(SURFACE_VARS)}
NO_SLIP, LAW, SOLID, IS_SET = 0x04000000, 0x08000000, 0x040000000, 0x080000000
TABLE = ("i", "j", "x", "y", "flags", "face_x", "face_y", "fric_x", "fric_y", "box_off")

DECKS = {
    "step": lambda: heat_keys(decks.step(37, 23, **BIG)),
    "wedge": lambda: heat_keys(decks.wedge15(67, 23, **BIG)),
    "resonator": lambda: heat_keys(decks.resonator(37, 23, **BIG)),
}


def flag_words(case):
    """[nx, ny] uint64: the flag word CT of every record."""
    rec = np.frombuffer(case.records(), dtype=np.uint8).reshape(-1, RECORD)
    return rec[:, CT_OFFSET:CT_OFFSET + 8].copy().view(np.uint64).reshape(case.nx, case.ny)   # (x-major records)


def node_flags(case):
    """[nx, ny] int: the table's flags of every cell by the issue's rule, 0 where the cell is no node."""
    ct = flag_words(case)
    has = lambda bit: (ct & np.uint64(bit)) != 0
    solid = has(SOLID)
    nb = np.zeros_like(solid)
    nb[1:, :] |= solid[:-1, :]
    nb[:-1, :] |= solid[1:, :]
    nb[:, 1:] |= solid[:, :-1]
    nb[:, :-1] |= solid[:, 1:]
    f = has(NO_SLIP) * 1 + has(LAW) * 2 + nb * 4
    return np.where(has(IS_SET) & ~solid, f, 0)


def in_box(case, i, j, box):
    """in_box of csrc/core/postproc.hpp: the reference's integer truncations."""
    x0, y0, dx, dy = box
    return (i >= int(x0 / case.dx)) & (i <= int((x0 + dx) / case.dx)) & (j >= int(y0 / case.dy)) & \
        (j <= int((y0 + dy) / case.dy))


def make_twin(sim, nsteps, **kw):
    """times [n], values [n, 10, nnodes] of a recorder-free run after each of its one-step calls."""
    times, vals = [], []
    for _ in range(nsteps):
        sim.step(1)
        sim.solver.download()
        vals.append(np.asarray(sim.case.surface(**kw)["values"]).copy())
        times.append(sim.summary()["time"])
    out = np.array(times), np.array(vals)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _twin(name):
    import openhyperflow2d_amd as hf

    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    return make_twin(sim, NSTEPS)


def stats_oracle(times, vals, t0, lo=0, hi=None, every=1, weight="time"):
    """The update rule of core/wall_heat.hpp over the twin's steps lo + 1 .. hi, armed at time t0."""
    hi = len(times) if hi is None else hi
    shape = vals.shape[1:]
    m, M, peak, pt = (np.zeros(shape) for _ in range(4))
    W, t_seen, samples = np.float64(0.0), np.float64(t0), 0
    for seen, k in enumerate(range(lo, hi), start=1):
        if seen % every:
            continue
        t = np.float64(times[k])
        w = np.float64(1.0) if weight == "step" else t - t_seen
        t_seen = t
        W1 = W + w
        r = w / W1 if W1 > 0 else np.float64(0.0)
        W = W1
        samples += 1
        v = vals[k].astype(np.float64)
        d = v - m
        m1 = m + r * d
        e = v - m1
        M = M + (w * d) * e
        m = m1
        upd = (v > peak) if samples > 1 else np.ones(shape, dtype=bool)
        peak = np.where(upd, v, peak)
        pt = np.where(upd, t, pt)
    var = M / W if samples else M
    return {"time": float(W), "samples": samples, "mean": m, "var": var, "peak": peak, "peak_time": pt}


def assert_history(h, times, vals, rows, what=""):
    """Bitwise: the history's rows are the twin's rows `rows` (indices into its steps)."""
    rows = list(rows)
    assert h["values"].shape == (len(rows),) + vals.shape[1:], (what, h["values"].shape)
    np.testing.assert_array_equal(h["times"], times[rows], err_msg=what)
    np.testing.assert_array_equal(h["values"], vals[rows], err_msg=what)
    # (the sign of a zero too: a friction term of size zero carries its neighbour's sign)
    np.testing.assert_array_equal(np.signbit(h["values"]), np.signbit(vals[rows]), err_msg=what)


def assert_stats(h, want, what=""):
    assert h["samples"] == want["samples"] and h["time"] == want["time"], (what, h["time"], want["time"])
    for k in ("mean", "var", "peak", "peak_time"):
        assert h[k].shape == want[k].shape and h[k].dtype == np.float64, (what, k)
        np.testing.assert_array_equal(h[k], want[k], err_msg="%s %s" % (what, k))


def assert_table(h, s, what=""):
    for k in TABLE:
        np.testing.assert_array_equal(h[k], s[k], err_msg="%s %s" % (what, k))


def stepped(hf, name, n=3):
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.step(n)
    sim.solver.download()
    return sim


def test_order_is_documented():
    assert SURFACE_VARS == ("p", "Cp", "T", "tau_x", "tau_y", "Cf_x", "Cf_y", "q_y", "q_x", "St")


@pytest.mark.parametrize("name", list(DECKS))
def test_oracle_unfolds_the_pressure_folds(hf, name):
    case = stepped(hf, name).case
    boxes, _ = targets(case)
    s = case.surface(boxes=boxes)
    v, off = s["values"], s["box_off"]
    assert v.shape == (10, len(s["i"])) and off[0] == 0 and off[-1] == len(s["i"]) and len(off) == len(boxes) + 1
    np.testing.assert_array_equal(v[V["p"]], np.asarray(case.field("p"))[s["i"], s["j"]])
    np.testing.assert_array_equal(v[V["T"]], np.asarray(case.field("T"))[s["i"], s["j"]])
    for b, box in enumerate(boxes):
        parts = case.force_parts(*box)
        for face, want, count in (("face_x", parts[0], parts[5]), ("face_y", parts[2], parts[7])):
            fold, n = np.float64(0.0), 0
            for k in range(off[b], off[b + 1]):
                if s[face][k] != 0:
                    fold += s[face][k] * v[V["p"], k]
                    n += 1
            assert n == count and fold == want, (name, b, face, fold, want)
    assert case.force_parts(*boxes[0])[5] > 0 and case.force_parts(*boxes[0])[7] > 0
    assert off[3] == off[2]   # the wall-free box holds no node


@pytest.mark.parametrize("name", list(DECKS))
def test_oracle_unfolds_the_friction_folds(hf, name):
    """(c m) g against c (m g): four roundings per term at the most, and n for the fold."""
    case = stepped(hf, name).case
    boxes, _ = targets(case)
    s = case.surface(boxes=boxes)
    v, off = s["values"], s["box_off"]
    for b, box in enumerate(boxes):
        parts = case.force_parts(*box)
        for fric, tau, want, count in (("fric_x", "tau_x", parts[1], parts[6]), ("fric_y", "tau_y", parts[3], parts[8])):
            k = np.arange(off[b], off[b + 1])
            k = k[s[fric][k] != 0]
            terms = s[fric][k] * v[V[tau], k]
            assert len(k) == count, (name, b, fric)
            fold = np.float64(0.0)
            for t in terms:
                fold += t
            bound = (len(k) + 4) * 2.0 ** -53 * np.abs(terms).sum()
            print("%s box %d %s: |diff| %.3e, bound %.3e over %d terms" % (name, b, fric, abs(fold - want), bound, len(k)))
            assert abs(fold - want) <= bound, (name, b, fric, fold, want)
    # Cf is tau over the dynamic pressure of the Cp flow; both are +0.0 where there is no friction term
    for t, c, f in (("tau_x", "Cf_x", "fric_x"), ("tau_y", "Cf_y", "fric_y")):
        none = s[f] == 0
        for a in (v[V[t]][none], v[V[c]][none]):
            assert not a.any() and not np.signbit(a).any()
        some = ~none & (v[V[t]] != 0)
        if some.any():
            q = v[V[t]][some] / v[V[c]][some]
            assert np.ptp(q) <= 4e-16 * abs(q).max() and q[0] > 0
    if name != "wedge":   # (the Euler wedge has no viscosity)
        assert (v[V["tau_x"]] != 0).any()


@pytest.mark.parametrize("name", list(DECKS))
def test_oracle_unfolds_the_heat_flux_profiles(hf, name):
    case = stepped(hf, name).case
    s = case.surface()
    v = s["values"]
    nx, ny = case.nx, case.ny
    y0, y1 = max(0, KEYS[2][1]), min(KEYS[3][1], ny - 1)
    slip = (s["flags"] & 1) != 0
    Qx, Qy = np.zeros(nx), np.zeros(ny)
    hits = 0
    for k in np.flatnonzero(slip):   # (i outer, j inner): each column's nodes in row order
        i, j = s["i"][k], s["j"][k]
        if y0 <= j < y1:
            q = v[V["q_y"], k]
            Qx[i] = max(Qx[i], q) if Qx[i] != 0 else q
            hits += 1
    for k in np.flatnonzero(slip):   # ... and each row's nodes in column order
        i, j = s["i"][k], s["j"][k]
        if i < nx - 1:
            q = v[V["q_x"], k]
            Qy[j] = max(Qy[j], q) if Qy[j] != 0 else q
    np.testing.assert_array_equal(Qx, np.asarray(case.heat_flux_x())[0])
    np.testing.assert_array_equal(Qy, np.asarray(case.heat_flux_y()))
    assert hits > 0 and Qx.any() and Qy.any()
    # St of the column's last node, Cp of every node
    last = {}
    for k in np.flatnonzero(slip):
        if y0 <= s["j"][k] < y1:
            last[s["i"][k]] = k
    full = np.asarray(case.heat_flux_x())
    for i, k in last.items():
        assert (v[V["Cp"], k], v[V["St"], k]) == (full[2, i], full[3, i])
    for q in ("q_y", "q_x", "St"):
        a = v[V[q]][~slip]
        assert not a.any() and not np.signbit(a).any()


@pytest.mark.parametrize("name", list(DECKS))
def test_node_table(hf, name):
    case = stepped(hf, name, 1).case
    s = case.surface()
    flags = node_flags(case)
    i, j = np.nonzero(flags)   # (row-major over [nx, ny]: i outer, j inner)
    np.testing.assert_array_equal(s["i"], i)
    np.testing.assert_array_equal(s["j"], j)
    np.testing.assert_array_equal(s["flags"], flags[i, j])
    np.testing.assert_array_equal(s["box_off"], [0, len(i)])
    # the coordinates of the field dump
    dx_out, dy_out = (case.dx * case.nx) / (case.nx - 1), (case.dy * case.ny) / (case.ny - 1)
    np.testing.assert_array_equal(s["x"], i * dx_out * 1.e3)
    np.testing.assert_array_equal(s["y"], dy_out * j * 1.e3)
    for k in ("face_x", "face_y", "fric_x", "fric_y"):
        z = s[k][(s["flags"] & 3) == 0]   # a slip node enters no load integral
        assert not z.any() and not np.signbit(z).any(), k
    assert (s["fric_x"] >= 0).all() and (s["fric_y"] <= 0).all() and (s["face_x"] != 0).any()
    # boxes: each list in (i, j) order by in_box; a node inside two boxes in both
    boxes, _ = targets(case)
    b = case.surface(boxes=boxes)
    want_i, want_j, off = [], [], [0]
    for box in boxes:
        keep = in_box(case, i, j, box)
        want_i += list(i[keep])
        want_j += list(j[keep])
        off.append(len(want_i))
    np.testing.assert_array_equal(b["i"], want_i)
    np.testing.assert_array_equal(b["j"], want_j)
    np.testing.assert_array_equal(b["box_off"], off)
    first = set(zip(b["i"][:off[1]], b["j"][:off[1]]))
    second = set(zip(b["i"][off[1]:off[2]], b["j"][off[1]:off[2]]))
    assert second and second <= first and off[1] == len(i)
    # a box around a single wall cell: one node, with the whole-field table's entries
    k = int(np.flatnonzero((s["flags"] & 3) != 0)[0])
    one = case.surface(boxes=[((s["i"][k] + 0.5) * case.dx, (s["j"][k] + 0.5) * case.dy, 0.0, 0.0)])
    assert len(one["i"]) == 1 and (one["i"][0], one["j"][0]) == (s["i"][k], s["j"][k])
    for key in TABLE[2:-1] + ("values",):
        np.testing.assert_array_equal(np.asarray(one[key]).T[0], np.asarray(s[key]).T[k], err_msg=key)


def slip_wedge():
    """The wedge with a slip (symmetry) condition on the body: no wall flag on any cell."""
    return decks.set_key(DECKS["wedge"](), "Contour1.Bound3.Cond", "NT_AX_2D")


def test_euler_slip_surface(hf):
    """The body of an Euler wedge with a slip wall: nodes with bit 2 only, p, Cp and T alone."""
    times, vals = [], []
    sim = hf.Simulation(slip_wedge(), "cpu")
    perturb(sim, SEED)
    sim.record_surface(capacity=8)
    twin = hf.Simulation(slip_wedge(), "cpu")
    perturb(twin, SEED)
    times, vals = make_twin(twin, 4)
    sim.step(4)
    h = sim.surface_history()
    assert_history(h, times, vals, range(4))
    assert len(h["flags"]) > 10 and (h["flags"] == 4).all()
    np.testing.assert_array_equal(h["flags"], node_flags(sim.case)[h["i"], h["j"]])
    for k in ("face_x", "face_y", "fric_x", "fric_y"):
        assert not h[k].any() and not np.signbit(h[k]).any()
    for q in SURFACE_VARS[3:]:
        assert not vals[:, V[q]].any()
    for q in SURFACE_VARS[:3]:
        assert (vals[1:, V[q]] != vals[:-1, V[q]]).any(), q
    assert twin.case.force_parts(0.0, 0.0, 1.0, 1.0)[5:] == (0, 0, 0, 0)   # the load integrals skip it


def test_no_nodes(hf):
    """A deck without nodes and a box without nodes: zero-length node axes, and a recorder that still ticks."""
    sim = hf.Simulation(heat_keys(decks.triple_point(160, 51, **BIG)), "cpu")
    perturb(sim, SEED)
    s = sim.case.surface()
    assert s["values"].shape == (10, 0) and all(len(s[k]) == 0 for k in TABLE[:-1]) and list(s["box_off"]) == [0, 0]
    sim.record_surface(capacity=4)
    sim.step(3)
    h = sim.surface_history()
    assert h["total"] == 3 and h["values"].shape == (3, 10, 0) and h["mean"].shape == (10, 0)
    assert (np.diff(h["times"]) > 0).all() and h["samples"] == 3
    wall = hf.Simulation(DECKS["step"](), "cpu")
    solid = np.asarray(wall.case.field("solid"))
    e = wall.case.surface(boxes=[empty_box(wall.case, solid)] * 2)
    assert e["values"].shape == (10, 0) and list(e["box_off"]) == [0, 0, 0]


@pytest.mark.parametrize("every,weight", [(1, "time"), (3, "step")])
@pytest.mark.parametrize("name", list(DECKS))
def test_recorder_equals_the_twin(hf, name, every, weight):
    times, vals = _twin(name)
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.record_surface(every=every, capacity=64, weight=weight)
    h = sim.surface_history()
    nn = vals.shape[2]
    assert h["total"] == 0 and h["samples"] == 0 and h["time"] == 0.0 and h["values"].shape == (0, 10, nn)
    assert not h["mean"].any() and not h["peak_time"].any() and nn > 0
    for n, res in [(1, False), (4, True), (7, False)]:
        sim.step(n, residual=res)
    h = sim.surface_history()
    rows = range(every - 1, NSTEPS, every)
    assert h["total"] == len(rows)
    assert_history(h, times, vals, rows, name)
    assert_stats(h, stats_oracle(times, vals, 0.0, every=every, weight=weight), name)
    assert_table(h, sim.case.surface(), name)
    # the peak is the largest sample and its time is that sample's
    np.testing.assert_array_equal(h["peak"], h["values"].max(axis=0))
    k = h["values"][:, V["p"]].argmax(axis=0)
    np.testing.assert_array_equal(h["peak_time"][V["p"]], h["times"][k])
    # recording moved nothing: the state is the twin's
    sim.solver.download()
    np.testing.assert_array_equal(sim.case.surface()["values"], vals[-1])
    # no comparison of constants
    assert (np.diff(times) > 0).all()
    for q in ("p", "T", "Cp", "q_y", "q_x", "St") + (() if name == "wedge" else ("tau_x", "Cf_x")):
        assert (vals[1:, V[q]] != vals[:-1, V[q]]).any(), q


def test_boxes_ring_wrap_statistics_only_and_clear(hf):
    name = "resonator"
    case = hf.Simulation(DECKS[name](), "cpu").case
    boxes, _ = targets(case)
    twin = hf.Simulation(DECKS[name](), "cpu")
    perturb(twin, SEED)
    times, vals = make_twin(twin, NSTEPS, boxes=boxes)
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.record_surface(boxes=boxes, capacity=7)
    sim.step(NSTEPS)
    h = sim.surface_history()
    assert h["total"] == NSTEPS and len(h["box_off"]) == 4 and h["box_off"][1] < h["box_off"][2]
    assert_history(h, times, vals, range(NSTEPS - 7, NSTEPS))
    assert_stats(h, stats_oracle(times, vals, 0.0))
    assert_table(h, sim.case.surface(boxes=boxes))
    # statistics only
    b = hf.Simulation(DECKS[name](), "cpu")
    perturb(b, SEED)
    b.record_surface(boxes=boxes, capacity=0, every=2)
    b.step(5)
    hb = b.surface_history()
    assert hb["total"] == 2 and hb["values"].shape == (0, 10, vals.shape[2]) and hb["times"].shape == (0,)
    assert_stats(hb, stats_oracle(times, vals, 0.0, hi=5, every=2))
    # clear: the ring, the statistics and the sampling count restart at the present time
    b.clear_surface()
    z = b.surface_history()
    assert z["total"] == 0 and z["samples"] == 0 and not z["mean"].any() and not z["peak"].any()
    b.step(4)
    assert_stats(b.surface_history(), stats_oracle(times, vals, times[4], lo=5, hi=9, every=2))
    # without statistics the keys are absent; arming again replaces the recorder
    b.record_surface(boxes=boxes, statistics=False, capacity=2)
    b.step(3)
    h = b.surface_history()
    assert "mean" not in h and "samples" not in h and h["total"] == 3
    assert_history(h, times, vals, range(10, 12))


def test_argument_errors_and_refusals(hf):
    sim = hf.Simulation(DECKS["wedge"](), "cpu")
    flows = sim.case.wall_heat_keys["flows"]
    box = (0.0, 0.0, 1.0, 1.0)
    nn = len(sim.case.surface()["i"])
    for kw in (dict(boxes=[box] * 17), dict(boxes=[(0.0, float("nan"), 1.0, 1.0)]), dict(boxes=[(0.0, 0.0, float("inf"), 1.0)]),
               dict(every=0), dict(capacity=-1), dict(weight="mass"), dict(cp_flow=0), dict(cp_flow=flows + 1),
               dict(capacity=0, statistics=False), dict(capacity=2 ** 31 // (10 * nn) + 1)):
        with pytest.raises(ValueError):
            sim.record_surface(**kw)
    for kw in (dict(boxes=[box] * 17), dict(boxes=[(0.0, float("nan"), 1.0, 1.0)]), dict(cp_flow=0), dict(cp_flow=flows + 1)):
        with pytest.raises(ValueError):
            sim.case.surface(**kw)
    with pytest.raises(RuntimeError):
        sim.surface_history()   # nothing armed: the refused calls left no recorder behind
    sim.record_surface(boxes=[box] * 16, capacity=2 ** 31 // (10 * 16 * nn))
    sim.step(1)
    assert sim.surface_history()["total"] == 1
    ref = hf.Simulation(DECKS["wedge"](), "ref")
    with pytest.raises(RuntimeError):
        ref.record_surface()


def test_a_strip_solver_refuses(hf):
    """One strip of several, built in-process without any collective."""
    for a, b in ((0, 30), (30, 67)):
        strip = hf.Simulation(DECKS["wedge"](), "cpu", gi0=a, gi1=b)
        with pytest.raises(RuntimeError, match="strip"):
            strip.record_surface()


def test_a_refused_rearm_leaves_the_recorder_whole(hf):
    """Armed, re-arms refused: the options, the ring and the statistics stay, also across an upload() that
    rebuilds the plan."""
    sim = hf.Simulation(DECKS["step"](), "cpu")
    perturb(sim, SEED)
    sim.record_surface(capacity=8, every=2)
    sim.step(4)
    before = sim.surface_history()
    for kw in (dict(cp_flow=sim.case.wall_heat_keys["flows"] + 1, capacity=3), dict(every=0), dict(boxes=[(0, 0, 1, 1)] * 17)):
        with pytest.raises(ValueError):
            sim.record_surface(**kw)
    after = sim.surface_history()
    assert before.keys() == after.keys() and after["total"] == 2
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    perturb(sim, SEED + 1)   # (set_records + upload: the plan is rebuilt over the same flags)
    sim.step(2)
    sim.solver.download()
    h = sim.surface_history()
    assert h["total"] == 3 and h["values"].shape[0] == 3
    np.testing.assert_array_equal(h["values"][-1], sim.case.surface()["values"])
    np.testing.assert_array_equal(h["values"][:2], before["values"])


def test_cli_surface(hf, tmp_path):
    text = decks.step(37, 23, nmax=6, nout=3)
    for k, v in [("MonitorIndex", 1), ("ExitMonitorValue", 1e-30)] + KEYS:
        text = decks.set_key(text, k, v)
    (tmp_path / "s.dat").write_text(text)
    out = tmp_path / "sf.npz"
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--cycles", "2", "--no-checkpoint",
            "--surface", str(out), "--surface-every", "2", "--surface-capacity", "2", timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    want = {"times", "values", "total", "mean", "var", "peak", "peak_time", "time", "samples", "vars"} | set(TABLE)
    assert want <= set(z.files)
    assert z["vars"].tolist() == list(SURFACE_VARS)
    case = hf.Simulation(text, "cpu").case
    boxes = case.load_targets[0]
    s = case.surface(boxes=boxes or None)
    nn = len(s["i"])
    assert nn > 0 and z["values"].shape == (2, 10, nn) and int(z["total"]) == 6 and int(z["samples"]) == 6
    for k in TABLE:
        np.testing.assert_array_equal(z[k], s[k], err_msg=k)
    assert (np.diff(z["times"]) > 0).all() and np.isfinite(z["values"]).all() and z["values"][:, V["q_y"]].any()
    assert z["mean"].shape == (10, nn)
    # a multi-rank launch is refused with a message, before anything runs
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--surface", str(tmp_path / "no.npz"),
            timeout=120, env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "one process" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "no.npz").exists()
