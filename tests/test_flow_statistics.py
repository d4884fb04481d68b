"""Time-averaged flow statistics (Simulation.start_averaging / averages) on
the CPU backend, which accumulates from its own arrays after every step.

The oracle is NumPy, never the code under test: a twin simulation of the same
backend and settings without an accumulator is advanced with step(1) and read
with field() and summary()["time"] after every step, and oracle() applies the
documented update rule to those arrays in float64,

    w = t_now - t_seen;  W1 = W + w;  r = w / W1;  W = W1
    d = x - m;  m = m + r * d;  e = x - m
    M = M + (w * d) * e;  C = C + (w * d_U) * e_V

with var = M / W and cov_uv = C / W.  Every comparison is bitwise.  All runs
start from tests.perturb.perturb, so no cell equals its neighbours."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.conftest import ROOT
from tests.perturb import SCHEDULE, perturb

SEED = 1
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
NSTEPS = sum(n for n, _ in SCHEDULE)

# name -> (deck text, Simulation keywords)
CPU_DECKS = {
    "wedge_lean": (lambda: decks.wedge15(40, 7, **BIG), {"lean": True}),
    "wedge_generic": (lambda: decks.wedge15(40, 7, **BIG), {"lean": False}),
    "step": (lambda: decks.step(37, 23, **BIG), {}),
}


def oracle(times, fields, solid, t0, lo=0, hi=None, every=1, second_moments=True, weight="time"):
    """The update rule over the twin's steps lo + 1 .. hi (rows lo .. hi - 1 of
    times [n] and fields {var: [n, nx, ny]}), armed at time t0; cells with
    solid != 0 stay 0."""
    hi = len(times) if hi is None else hi
    gas = np.asarray(solid) == 0.0
    shape = (len(PROBE_VARS),) + gas.shape
    m, M, C = np.zeros(shape), np.zeros(shape), np.zeros(gas.shape)
    W, t_seen, samples = np.float64(0.0), np.float64(t0), 0
    for seen, k in enumerate(range(lo, hi), start=1):
        if seen % every:
            continue
        t_now = np.float64(times[k])
        w = np.float64(1.0) if weight == "step" else t_now - t_seen
        t_seen = t_now
        W1 = W + w
        r = w / W1
        W = W1
        samples += 1
        x = np.array([fields[v][k] for v in PROBE_VARS], dtype=np.float64)
        d = x - m
        m1 = m + r * d
        e = x - m1
        m = np.where(gas, m1, 0.0)
        M = np.where(gas, M + (w * d) * e, 0.0)
        C = np.where(gas, C + (w * d[3]) * e[4], 0.0)
    out = {"mean": m, "time": float(W), "samples": samples}
    if second_moments:
        out["var"] = M / W if samples else M
        out["cov_uv"] = C / W if samples else C
    return out


def assert_equals_oracle(got, want, cols=None, what=""):
    """Bitwise: mean / var / cov_uv over the columns got["columns"], time, samples."""
    a, b = got["columns"] if cols is None else cols
    assert got["samples"] == want["samples"], what
    assert got["time"] == want["time"], (what, got["time"], want["time"])
    keys = [k for k in ("mean", "var", "cov_uv") if k in want]
    assert sorted(k for k in got if k in ("mean", "var", "cov_uv")) == sorted(keys), what
    for k in keys:
        w = want[k][..., a:b, :]
        assert got[k].shape == w.shape, (what, k, got[k].shape, w.shape)
        np.testing.assert_array_equal(got[k], w, err_msg="%s %s" % (what, k))


def _sim(hf, name, **kw):
    gen, skw = CPU_DECKS[name]
    s = hf.Simulation(gen(), "cpu", **dict(skw, **kw))
    perturb(s, SEED)
    return s


@functools.lru_cache(maxsize=None)
def _twin(name, gi0=0, gi1=-1):
    """(t0, times [14], fields {var: [14, nx, ny]}, solid) of the accumulator-free
    twin over SCHEDULE, one step per call (computed once, read-only)."""
    import openhyperflow2d_amd as hf

    s = _sim(hf, name, gi0=gi0, gi1=gi1)
    t0 = s.summary()["time"]
    solid = np.asarray(s.field("solid")).copy()
    times, fields = [], {v: [] for v in PROBE_VARS}
    for n, res in SCHEDULE:
        for k in range(n):
            s.step(1, residual=res and k == n - 1)
            for v in PROBE_VARS:
                fields[v].append(np.asarray(s.field(v)).copy())
            times.append(s.summary()["time"])
    out = {v: np.array(a) for v, a in fields.items()}
    for a in list(out.values()) + [solid]:
        a.setflags(write=False)
    return t0, np.array(times), out, solid


def test_vars_order_is_the_recorders():
    assert PROBE_VARS == ("p", "T", "rho", "U", "V")


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("weight", ["time", "step"])
@pytest.mark.parametrize("name", list(CPU_DECKS))
def test_averages_equal_the_oracle(hf, name, weight, every):
    a = _sim(hf, name)
    a.start_averaging(every=every, weight=weight)
    zero = a.averages()
    assert zero["time"] == 0.0 and zero["samples"] == 0
    assert not zero["mean"].any() and not zero["var"].any() and not zero["cov_uv"].any()
    for n, res in SCHEDULE:
        a.step(n, residual=res)
    got = a.averages()
    t0, times, fields, solid = _twin(name)
    want = oracle(times, fields, solid, t0, every=every, weight=weight)
    nx, ny = solid.shape
    assert NSTEPS == 14 and got["samples"] == (14 if every == 1 else 4)
    assert got["columns"] == (0, nx) and got["mean"].shape == (5, nx, ny) and got["cov_uv"].shape == (nx, ny)
    assert_equals_oracle(got, want, what=name)
    if weight == "step":
        assert got["time"] == got["samples"]
    else:
        # W is the averaged span: a sum of at most 14 differences of the clock
        assert abs(got["time"] - (times[14 - 14 % every - 1] - t0)) <= 14 * np.spacing(got["time"])
    # the statistics are not trivial: the field moved, and the variables differ
    gas = solid == 0.0
    assert (got["var"] >= 0).all() and (got["var"][:, gas] > 0).mean() > 0.5 and (got["cov_uv"][gas] != 0).any()
    assert not np.array_equal(got["mean"][3], got["mean"][4])
    # accumulating leaves the run unchanged
    b = _sim(hf, name)
    for n, res in SCHEDULE:
        b.step(n, residual=res)
    for f in PROBE_VARS + ("k", "R", "CP"):
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)
    assert a.summary()["dt"] == b.summary()["dt"] and a.summary()["time"] == b.summary()["time"]
    assert_equals_oracle(a.averages(), want, what="read twice")


def test_mean_only(hf):
    a = _sim(hf, "wedge_lean")
    a.start_averaging(second_moments=False)
    for n, res in SCHEDULE:
        a.step(n, residual=res)
    got = a.averages()
    t0, times, fields, solid = _twin("wedge_lean")
    assert "var" not in got and "cov_uv" not in got
    assert_equals_oracle(got, oracle(times, fields, solid, t0, second_moments=False))


def test_solid_cells_stay_zero_and_columns(hf):
    t0, times, fields, solid = _twin("step")
    assert (solid != 0.0).any()
    a = _sim(hf, "step")
    a.start_averaging()
    a.step(5)
    got = a.averages()
    for k in ("mean", "var"):
        assert not got[k][:, solid != 0.0].any(), k
    assert not got["cov_uv"][solid != 0.0].any()
    assert (got["mean"][2][solid == 0.0] > 0).all()   # every gas cell has a density
    # a solver of a column sub-range: its own columns only
    nx = solid.shape[0]
    g0, g1 = nx // 3, nx - 5
    s = _sim(hf, "step", gi0=g0, gi1=g1)
    s.start_averaging()
    for n, res in SCHEDULE:
        s.step(n, residual=res)
    got = s.averages()
    assert got["columns"] == (g0, g1) and got["mean"].shape == (5, g1 - g0, solid.shape[1])
    t0, times, fields, solid = _twin("step", g0, g1)
    assert_equals_oracle(got, oracle(times, fields, solid, t0), what="sub-range")


def test_lifecycle(hf):
    t0, times, fields, solid = _twin("wedge_lean")
    a = _sim(hf, "wedge_lean")
    with pytest.raises(RuntimeError):
        a.averages()   # nothing armed
    with pytest.raises(ValueError):
        a.start_averaging(every=0)
    with pytest.raises(ValueError):
        a.start_averaging(weight="mass")
    with pytest.raises(RuntimeError):
        a.averages()   # the refused calls left no accumulator behind
    a.start_averaging()
    a.step(5)
    assert_equals_oracle(a.averages(), oracle(times, fields, solid, t0, 0, 5), what="first five")
    # reset: the later steps only, weighted from the reset
    a.reset_averaging()
    z = a.averages()
    assert z["samples"] == 0 and z["time"] == 0.0 and not z["mean"].any() and not z["var"].any()
    a.step(6)
    want = oracle(times, fields, solid, times[4], 5, 11)
    assert_equals_oracle(a.averages(), want, what="after reset")
    # stop: frozen
    a.stop_averaging()
    a.step(3)
    assert_equals_oracle(a.averages(), want, what="stopped")
    np.testing.assert_array_equal(a.field("p"), fields["p"][13])
    # starting again with other options restarts from zero
    a.start_averaging(every=2, second_moments=False, weight="step")
    z = a.averages()
    assert z["samples"] == 0 and "var" not in z and not z["mean"].any()
    ref = hf.Simulation(CPU_DECKS["wedge_lean"][0](), "ref")
    with pytest.raises(RuntimeError):
        ref.start_averaging()


def _py(*args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", *args], capture_output=True, text=True,
                          env=env, **kw)


def test_cli_averages(hf, tmp_path):
    text = decks.wedge15(40, 12, nmax=6, nout=3)
    text = decks.set_key(decks.set_key(text, "MonitorIndex", 1), "ExitMonitorValue", 1e-30)
    outs = {}
    for tag in ("plain", "avg"):
        d = tmp_path / tag
        d.mkdir()
        (d / "w.dat").write_text(text)
        extra = ["--averages", str(tmp_path / "avg.npz"), "--averages-every", "2"] if tag == "avg" else []
        r = _py("run", str(d / "w.dat"), "--backend", "cpu", "--cycles", "2", "--no-checkpoint", *extra, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs[tag] = {f.name: f.read_bytes() for f in sorted(d.iterdir()) if f.is_file()}
    z = np.load(tmp_path / "avg.npz")
    assert set(z.files) == {"mean", "var", "cov_uv", "vars", "time", "samples"}
    assert z["vars"].tolist() == list(PROBE_VARS)
    # the same run in this process
    d = tmp_path / "here"
    d.mkdir()
    sim = hf.Simulation(text, "cpu", workdir=str(d), use_checkpoint=False, lean=True)
    sim.start_averaging(every=2)
    sim.run(max_cycles=2, outdir=str(d), outputs=True, checkpoint=False, verbose=False)
    av = sim.averages()
    assert int(z["samples"]) == av["samples"] == 6 and float(z["time"]) == av["time"] > 0
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(z[k], av[k], err_msg=k)
    assert z["mean"].shape == (5, 40, 12)
    # the driver's own outputs do not know about the flag
    assert len(outs["plain"]) > 1 and outs["plain"].keys() == outs["avg"].keys()
    for name, data in outs["plain"].items():
        assert outs["avg"][name] == data, name
    # a multi-rank launch is refused with a message, before anything runs
    r = subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", "run", str(tmp_path / "plain" / "w.dat"),
                        "--backend", "cpu", "--averages", str(tmp_path / "no.npz")], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and "one process" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "no.npz").exists()
