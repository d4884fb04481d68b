"""Per-step wall heat recorder (Simulation.record_wall_heat / wall_heat_history)
and its oracles Case.heat_flux_x / heat_flux_y on the CPU backend, which
evaluates the shared plan (core/wall_heat.hpp) on its own arrays after every
step.

The oracles are pinned to the writer: every value formatted with '%g' is the
token save_heat_flux writes.  The recorder's oracle is a twin simulation
without a recorder, advanced with step(1), downloaded after every step and read
through Case.heat_flux_x / heat_flux_y and summary()["time"] (computed once per
deck, shared, never modified); the statistics' oracle is the update rule
transcribed in NumPy over the twin's profiles and times.  Every comparison is
bitwise.  All runs start from tests.perturb.perturb."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import WALL_HEAT_X
from tests.conftest import ROOT
from tests.perturb import RECORD, perturb

SEED = 1
CT_OFFSET = 384   # of the flag word CT in a cell record
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
KEYS = [("isOutHeatFluxX", 1), ("Cp_Flow_Index", 1), ("y_min", 0), ("y_max", 1000), ("isOutHeatFluxY", 1)]
WALL_NO_SLIP = 0x04000000   # CT_WALL_NO_SLIP: a node of both profiles
NSTEPS = 12


def heat_keys(text, keys=KEYS):
    """The deck with the heat-flux keys of the protocol set."""
    for k, v in keys:
        text = decks.set_key(text, k, v)
    return text


DECKS = {
    "step": lambda: heat_keys(decks.step(37, 23, **BIG)),
    "resonator": lambda: heat_keys(decks.resonator(37, 23, **BIG)),
    "scramjet": lambda: heat_keys(decks.scramjet(37, 23, **BIG)),
    "wedge": lambda: heat_keys(decks.wedge15(67, 23, **BIG)),
}
# columns and rows that hold at least one node (measured on the CPU backend)
HOLD = {"step": (30, 4), "resonator": (34, 23), "scramjet": (33, 11), "wedge": (47, 11)}


def profiles(case, **kw):
    """(x [4, nx], y [ny]) of the case's records through the oracles."""
    return np.asarray(case.heat_flux_x(**kw)), np.asarray(case.heat_flux_y())


def walls(case):
    """[nx, ny] bool: the CT_WALL_NO_SLIP cells."""
    rec = np.frombuffer(case.records(), dtype=np.uint8).reshape(-1, RECORD)
    ct = rec[:, CT_OFFSET:CT_OFFSET + 8].copy().view(np.uint64).reshape(case.nx, case.ny)   # (x-major records)
    return (ct & np.uint64(WALL_NO_SLIP)) != 0


def node_counts(case, rows=None):
    """(x_nodes [nx], y_nodes [ny]) as heat_flux_x_cols / heat_flux_y_terms walk the grid."""
    w = walls(case)
    nx, ny = w.shape
    y0, y1 = (0, 1000) if rows is None else rows
    return w[:, max(0, y0):min(y1, ny - 1)].sum(axis=1), w[:nx - 1, :].sum(axis=0)


def make_twin(sim, nsteps):
    """times [n], x [n, 4, nx], y [n, ny] of a recorder-free run after each of its one-step calls."""
    times, xs, ys = [], [], []
    for _ in range(nsteps):
        sim.step(1)
        sim.solver.download()
        x, y = profiles(sim.case)
        xs.append(x.copy())
        ys.append(y.copy())
        times.append(sim.summary()["time"])
    out = np.array(times), np.array(xs), np.array(ys)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _twin(name):
    import openhyperflow2d_amd as hf

    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    return make_twin(sim, NSTEPS)


def stats_oracle(times, x, y, t0, lo=0, hi=None, every=1, weight="time"):
    """The update rule of core/wall_heat.hpp over the twin's steps lo + 1 .. hi, armed at time t0."""
    hi = len(times) if hi is None else hi
    n, _, nx = x.shape
    prof = np.concatenate([x.reshape(n, 4 * nx), y], axis=1).astype(np.float64)
    ne = prof.shape[1]
    m, M, peak, pt = np.zeros(ne), np.zeros(ne), np.zeros(ne), np.zeros(ne)
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
        v = prof[k]
        d = v - m
        m1 = m + r * d
        e = v - m1
        M = M + (w * d) * e
        m = m1
        upd = (v > peak) if samples > 1 else np.ones(ne, dtype=bool)
        peak = np.where(upd, v, peak)
        pt = np.where(upd, t, pt)
    var = M / W if samples else M
    out = {"time": float(W), "samples": samples}
    for key, a in (("mean", m), ("var", var), ("peak", peak), ("peak_time", pt)):
        out[key + "_x"] = a[:4 * nx].reshape(4, nx)
        out[key + "_y"] = a[4 * nx:]
    return out


def assert_history(h, times, x, y, rows, what=""):
    """Bitwise: the history's rows are the twin's rows `rows` (indices into its steps)."""
    rows = list(rows)
    assert h["x"].shape == (len(rows),) + x.shape[1:] and h["y"].shape == (len(rows), y.shape[1]), what
    np.testing.assert_array_equal(h["times"], times[rows], err_msg=what)
    np.testing.assert_array_equal(h["x"], x[rows], err_msg=what)
    np.testing.assert_array_equal(h["y"], y[rows], err_msg=what)


def assert_stats(h, want, what=""):
    assert h["samples"] == want["samples"] and h["time"] == want["time"], (what, h["time"], want["time"])
    for k, v in want.items():
        if k not in ("time", "samples"):
            assert h[k].shape == v.shape and h[k].dtype == np.float64, (what, k)
            np.testing.assert_array_equal(h[k], v, err_msg="%s %s" % (what, k))


def test_order_is_documented():
    assert WALL_HEAT_X == ("Q", "Alpha", "Cp", "St")


@pytest.mark.parametrize("name", list(DECKS))
def test_oracles_equal_the_pinned_writer(hf, tmp_path, name):
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.step(3)
    sim.solver.download()
    x, y = profiles(sim.case)
    nx, ny = sim.case.nx, sim.case.ny
    assert x.shape == (4, nx) and y.shape == (ny,)
    px, py = tmp_path / "x.plt", tmp_path / "y.plt"
    sim.case.save_heat_flux(str(px), str(py))
    tx = [ln.split() for ln in px.read_text().splitlines()[1:]]
    ty = [ln.split() for ln in py.read_text().splitlines()[1:]]
    assert len(tx) == nx and len(ty) == ny
    for i in range(nx):
        assert tx[i][1:] == ["%g" % v for v in x[:, i]], (name, i)
    for j in range(ny):
        assert ty[j][1] == "%g" % y[j], (name, j)
    xn, yn = node_counts(sim.case)
    assert (int((xn > 0).sum()), int((yn > 0).sum())) == HOLD[name]
    assert (x[:, xn == 0] == 0).all() and (y[yn == 0] == 0).all()
    assert np.isfinite(x).all() and np.isfinite(y).all() and (x[1, xn > 0] > 0).all()


def test_explicit_arguments_equal_the_deck_keys(hf):
    plain = hf.Simulation(decks.resonator(37, 23, **BIG), "cpu")   # the generator's own keys: no X profile
    keyed = hf.Simulation(heat_keys(decks.resonator(37, 23, **BIG), KEYS[:2] + [("y_min", 3), ("y_max", 14)] + KEYS[4:]),
                          "cpu")
    for s in (plain, keyed):
        perturb(s, SEED)
        s.step(2)
        s.solver.download()
    x, y = profiles(keyed.case)
    np.testing.assert_array_equal(plain.case.heat_flux_x(cp_flow=1, rows=(3, 14)), x)
    np.testing.assert_array_equal(plain.case.heat_flux_y(), y)
    # narrower rows change the X profile only
    wide = np.asarray(keyed.case.heat_flux_x(rows=(0, 1000)))
    assert (wide != x).any()
    np.testing.assert_array_equal(keyed.case.heat_flux_y(), y)
    xn, _ = node_counts(keyed.case, rows=(3, 14))
    assert (x[:, xn == 0] == 0).all() and (x[1, xn > 0] > 0).all() and (xn > 0).any()
    for bad in (0, keyed.case.wall_heat_keys["flows"] + 1, -1):
        with pytest.raises(ValueError):
            keyed.case.heat_flux_x(cp_flow=bad)


@pytest.mark.parametrize("every,weight", [(1, "time"), (3, "step")])
@pytest.mark.parametrize("name", list(DECKS))
def test_recorder_equals_the_twin(hf, name, every, weight):
    times, x, y = _twin(name)
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.record_wall_heat(every=every, capacity=64, weight=weight)
    h = sim.wall_heat_history()
    assert h["total"] == 0 and h["samples"] == 0 and h["time"] == 0.0 and h["x"].shape == (0, 4, sim.case.nx)
    assert not h["mean_x"].any() and not h["peak_time_y"].any()
    for n, res in [(1, False), (4, True), (7, False)]:
        sim.step(n, residual=res)
    h = sim.wall_heat_history()
    rows = range(every - 1, NSTEPS, every)
    assert h["total"] == len(rows)
    assert_history(h, times, x, y, rows, name)
    assert_stats(h, stats_oracle(times, x, y, 0.0, every=every, weight=weight), name)
    xn, yn = node_counts(sim.case)
    np.testing.assert_array_equal(h["x_nodes"], xn)
    np.testing.assert_array_equal(h["y_nodes"], yn)
    # the peak is the largest sample and its time is that sample's
    np.testing.assert_array_equal(h["peak_x"], h["x"].max(axis=0))
    k = h["y"].argmax(axis=0)
    np.testing.assert_array_equal(h["peak_time_y"], h["times"][k])
    # recording moved nothing: the state is the twin's
    sim.solver.download()
    fx, fy = profiles(sim.case)
    np.testing.assert_array_equal(fx, x[-1])
    np.testing.assert_array_equal(fy, y[-1])


@pytest.mark.parametrize("name", list(DECKS))
def test_the_twin_is_no_comparison_of_constants(hf, name):
    """Q, Cp, St and the Y profile change between steps; some list holds two
    nodes or more; both arms of the max-or-first rule are taken."""
    times, x, y = _twin(name)
    assert (np.diff(times) > 0).all()
    for v in (0, 2, 3):
        assert (x[1:, v] != x[:-1, v]).any(), WALL_HEAT_X[v]
    assert (y[1:] != y[:-1]).any()
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.step(2)
    sim.solver.download()
    case = sim.case
    w = walls(case)
    xn, yn = node_counts(case)
    if name == "step":
        assert ((xn >= 2).sum(), (yn >= 2).sum()) == (1, 1)
    if name == "resonator":
        assert ((xn >= 2).sum(), (yn >= 2).sum()) == (7, 4)
    full = np.asarray(case.heat_flux_x())
    one = lambda i, j: np.asarray(case.heat_flux_x(rows=(j, j + 1)))[:, i]   # the term of node (i, j) alone
    first = max_arm = 0
    for i in np.flatnonzero(xn > 0):
        js = [j for j in np.flatnonzero(w[i]) if j < case.ny - 1]
        Q, Al = 0.0, 0.0
        for j in js:   # the rule, over the single nodes' terms
            q, al = one(i, j)[:2]
            if Q != 0:
                Q, Al = max(Q, q), max(Al, al)
                max_arm += 1
            else:
                Q, Al = q, al
                first += 1
        assert (Q, Al) == (full[0, i], full[1, i])
        np.testing.assert_array_equal(one(i, js[-1])[2:], full[2:, i])   # Cp, St: the last node's
    assert first > 0
    if name in ("step", "resonator"):
        assert max_arm > 0


def test_ring_wrap_statistics_only_and_clear(hf):
    name = "resonator"
    times, x, y = _twin(name)
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.record_wall_heat(capacity=7)
    sim.step(NSTEPS)
    h = sim.wall_heat_history()
    assert h["total"] == NSTEPS
    assert_history(h, times, x, y, range(NSTEPS - 7, NSTEPS))
    assert_stats(h, stats_oracle(times, x, y, 0.0))
    # statistics only
    b = hf.Simulation(DECKS[name](), "cpu")
    perturb(b, SEED)
    b.record_wall_heat(capacity=0, every=2)
    b.step(5)
    hb = b.wall_heat_history()
    assert hb["total"] == 2 and hb["x"].shape == (0, 4, b.case.nx) and hb["times"].shape == (0,)
    assert_stats(hb, stats_oracle(times, x, y, 0.0, hi=5, every=2))
    # clear: the ring, the statistics and the sampling count restart at the present time
    b.clear_wall_heat()
    z = b.wall_heat_history()
    assert z["total"] == 0 and z["samples"] == 0 and not z["mean_x"].any() and not z["peak_y"].any()
    b.step(4)
    assert_stats(b.wall_heat_history(), stats_oracle(times, x, y, times[4], lo=5, hi=9, every=2))
    # without statistics the keys are absent; arming again replaces the recorder
    b.record_wall_heat(statistics=False, capacity=2)
    b.step(3)
    h = b.wall_heat_history()
    assert "mean_x" not in h and "samples" not in h and h["total"] == 3
    assert_history(h, times, x, y, range(10, 12))


def test_one_profile_alone(hf):
    name = "step"
    times, x, y = _twin(name)
    for kw, keep in ((dict(x=False), "y"), (dict(y=False), "x")):
        sim = hf.Simulation(DECKS[name](), "cpu")
        perturb(sim, SEED)
        sim.record_wall_heat(**kw)
        sim.step(3)
        h = sim.wall_heat_history()
        np.testing.assert_array_equal(h[keep], (x if keep == "x" else y)[:3])
        other = "x" if keep == "y" else "y"
        assert not h[other].any() and not np.signbit(h[other]).any() and not h[other + "_nodes"].any()
        assert h[keep + "_nodes"].any()


def test_empty_lists(hf):
    """No node anywhere: every profile is +0.0, every count 0."""
    sim = hf.Simulation(heat_keys(decks.triple_point(160, 51, **BIG)), "cpu")
    perturb(sim, SEED)
    sim.record_wall_heat(capacity=4)
    sim.step(3)
    sim.solver.download()
    h = sim.wall_heat_history()
    x, y = profiles(sim.case)
    assert h["total"] == 3 and h["x"].shape == (3, 4, 160) and h["y"].shape == (3, 51)
    for a in (x, y, h["x"], h["y"], h["mean_x"], h["var_y"], h["peak_x"], h["peak_y"]):
        assert not a.any() and not np.signbit(a).any()
    assert not h["x_nodes"].any() and not h["y_nodes"].any()
    assert (np.diff(h["times"]) > 0).all()


def test_refusals(hf):
    sim = hf.Simulation(DECKS["wedge"](), "cpu")
    flows = sim.case.wall_heat_keys["flows"]
    for kw in (dict(x=False, y=False), dict(every=0), dict(capacity=-1), dict(weight="mass"), dict(cp_flow=0),
               dict(cp_flow=flows + 1), dict(capacity=0, statistics=False)):
        with pytest.raises(ValueError):
            sim.record_wall_heat(**kw)
    with pytest.raises(RuntimeError):
        sim.wall_heat_history()   # nothing armed: the refused calls left no recorder behind
    sim.record_wall_heat(x=False, cp_flow=flows + 1)   # the Y profile reads no flow
    sim.step(1)
    assert sim.wall_heat_history()["total"] == 1
    ref = hf.Simulation(DECKS["wedge"](), "ref")
    with pytest.raises(RuntimeError):
        ref.record_wall_heat()


def test_a_strip_solver_refuses(hf):
    """One strip of several, built in-process without any collective."""
    for a, b in ((0, 30), (30, 67)):
        strip = hf.Simulation(DECKS["wedge"](), "cpu", gi0=a, gi1=b)
        with pytest.raises(RuntimeError, match="strip"):
            strip.record_wall_heat()


def test_a_refused_rearm_leaves_the_recorder_whole(hf):
    """Armed, re-arms refused: the options, the ring and the statistics stay, also across an upload() that
    rebuilds the plan."""
    name = "step"
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    sim.record_wall_heat(capacity=8, every=2)
    sim.step(4)
    before = sim.wall_heat_history()
    with pytest.raises(ValueError):
        sim.record_wall_heat(cp_flow=sim.case.wall_heat_keys["flows"] + 1, capacity=3)
    with pytest.raises(ValueError):
        sim.record_wall_heat(every=0)
    after = sim.wall_heat_history()
    assert before.keys() == after.keys() and after["total"] == 2
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    perturb(sim, SEED + 1)   # (set_records + upload: the plan is rebuilt)
    sim.step(2)
    sim.solver.download()
    h = sim.wall_heat_history()
    x, y = profiles(sim.case)
    assert h["total"] == 3 and h["x"].shape == (3, 4, sim.case.nx)
    np.testing.assert_array_equal(h["x"][-1], x)
    np.testing.assert_array_equal(h["y"][-1], y)


def _py(*args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.update(kw.pop("env", {}))
    return subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", *args], capture_output=True, text=True,
                          env=env, **kw)


def test_cli_wall_heat(hf, tmp_path):
    text = decks.step(37, 23, nmax=6, nout=3)
    for k, v in [("MonitorIndex", 1), ("ExitMonitorValue", 1e-30)] + KEYS:
        text = decks.set_key(text, k, v)
    (tmp_path / "s.dat").write_text(text)
    out = tmp_path / "wq.npz"
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--cycles", "2", "--no-checkpoint",
            "--wall-heat", str(out), "--wall-heat-every", "2", "--wall-heat-capacity", "4", timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    want = {"times", "x", "y", "total", "x_nodes", "y_nodes", "time", "samples", "vars"}
    want |= {s + "_" + p for s in ("mean", "var", "peak", "peak_time") for p in ("x", "y")}
    assert want <= set(z.files)
    assert z["vars"].tolist() == list(WALL_HEAT_X)
    assert z["x"].shape == (4, 4, 37) and z["y"].shape == (4, 23) and int(z["total"]) == 6 and int(z["samples"]) == 6
    assert (np.diff(z["times"]) > 0).all() and np.isfinite(z["x"]).all() and z["x"].any() and z["y"].any()
    assert z["mean_x"].shape == (4, 37) and z["peak_time_y"].shape == (23,)
    # X is recorded only when the deck asks for HeatFlux-X
    (tmp_path / "y.dat").write_text(decks.set_key(text, "isOutHeatFluxX", 0))
    r = _py("run", str(tmp_path / "y.dat"), "--backend", "cpu", "--cycles", "1", "--no-checkpoint",
            "--wall-heat", str(tmp_path / "y.npz"), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(tmp_path / "y.npz")
    assert not z["x"].any() and not z["x_nodes"].any() and z["y"].any()
    # a multi-rank launch is refused with a message, before anything runs
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--wall-heat", str(tmp_path / "no.npz"),
            timeout=120, env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "one process" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "no.npz").exists()
