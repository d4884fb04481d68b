"""Field frames: the oracle Case.frame and the per-step recorder
Simulation.record_frames / frame_history on the CPU backend, which evaluates the
shared rule (core/frame_rule.hpp) on its own arrays after every step.

The oracle is pinned twice: bit for bit to an independent NumPy transcription of
the rule over case.field(...), and to analytic fields written into the records
(a linear density, a solid-body rotation, a uniform expansion), so that one
mistake transcribed twice still shows.  The recorder's oracle is a twin
simulation without a recorder, advanced with step(1), downloaded after every
step and read through Case.frame and summary()["time"] (computed once per deck,
shared, never modified).  Every comparison with the twin is bitwise.  All runs
start from tests.perturb.perturb."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import FRAME_VARS, PROBE_VARS
from tests.fp32_cases import REC64
from tests.perturb import perturb
from tests.test_wall_heat import _py

SEED = 1
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
NSTEPS = 26
SOLID, IS_SET = np.uint64(0x040000000), np.uint64(0x080000000)
V = {name: k for k, name in enumerate(FRAME_VARS)}
STATIC = ("vars", "i", "j", "x", "y", "gas")

DECKS = {
    "wedge": lambda: decks.wedge15(67, 23, **BIG),
    "step": lambda: decks.step(37, 23, **BIG),
    "triple_point": lambda: decks.triple_point(48, 24, **BIG),
}


def gas_of(case):
    ct = np.asarray(case.field("CT")).astype(np.uint64)
    return ((ct & IS_SET) != 0) & ((ct & SOLID) == 0)


def neighbour_flags(gas):
    hasW, hasE, hasS, hasN = (np.zeros_like(gas) for _ in range(4))
    hasW[1:, :] = gas[:-1, :]
    hasE[:-1, :] = gas[1:, :]
    hasS[:, 1:] = gas[:, :-1]
    hasN[:, :-1] = gas[:, 1:]
    return hasW, hasE, hasS, hasN


def numpy_frame(case):
    """[10, nx, ny]: the rule of the issue over case.field(...), in float64, one operation per rounding."""
    q = {v: np.asarray(case.field(v), dtype=np.float64) for v in PROBE_VARS}
    gas = gas_of(case)
    hasW, hasE, hasS, hasN = neighbour_flags(gas)
    ix = (1.0 / np.float64(case.dx)) / np.maximum(hasW.astype(np.int64) + hasE, 1).astype(np.float64)
    iy = (1.0 / np.float64(case.dy)) / np.maximum(hasS.astype(np.int64) + hasN, 1).astype(np.float64)

    def ddx(a):
        e = np.where(hasE, np.roll(a, -1, axis=0), a)
        w = np.where(hasW, np.roll(a, 1, axis=0), a)
        return (e - w) * ix

    def ddy(a):
        n = np.where(hasN, np.roll(a, -1, axis=1), a)
        s = np.where(hasS, np.roll(a, 1, axis=1), a)
        return (n - s) * iy

    def mag(a):
        gx, gy = ddx(a), ddy(a)
        return np.sqrt(gx * gx + gy * gy)

    om = ddx(q["V"]) - ddy(q["U"])
    th = ddx(q["U"]) + ddy(q["V"])
    t2, o2 = th * th, om * om
    out = [q[v] for v in PROBE_VARS] + [mag(q["rho"]), mag(q["p"]), om, th, t2 / ((t2 + o2) + 1e-30)]
    return np.array([np.where(gas, a, 0.0) for a in out])


def same_bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape, msg)
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64), err_msg=msg)


def _sim(hf, name, steps=0):
    s = hf.Simulation(DECKS[name](), "cpu")
    perturb(s, SEED)
    if steps:
        s.step(steps)
        s.solver.download()
    return s


def test_frame_vars():
    assert FRAME_VARS == ("p", "T", "rho", "U", "V", "grad_rho", "grad_p", "vorticity", "dilatation", "ducros")
    assert FRAME_VARS[:5] == PROBE_VARS


@pytest.mark.parametrize("name", list(DECKS))
def test_oracle_equals_the_numpy_rule(hf, name):
    sim = _sim(hf, name, steps=3)
    case = sim.case
    f = case.frame()
    want = numpy_frame(case)
    assert tuple(f["vars"]) == FRAME_VARS and f["values"].shape == (10, case.nx, case.ny)
    for v, var in enumerate(FRAME_VARS):
        same_bits(f["values"][v], want[v], var)
    gas = gas_of(case)
    np.testing.assert_array_equal(f["gas"], gas)
    np.testing.assert_array_equal(f["i"], np.arange(case.nx))
    np.testing.assert_array_equal(f["j"], np.arange(case.ny))
    assert f["x"].shape == (case.nx,) and f["y"].shape == (case.ny,) and (np.diff(f["x"]) > 0).all()
    # the row variables are field(name); nothing compares constants
    for var in PROBE_VARS:
        same_bits(f["values"][V[var]], np.where(gas, case.field(var), 0.0), var)
    for var in FRAME_VARS[5:]:
        a = f["values"][V[var]][gas]
        assert np.isfinite(a).all() and a.min() != a.max(), var
    assert (f["values"][V["ducros"]] >= 0).all() and (f["values"][V["ducros"]] <= 1).all()
    if name == "wedge":   # every stencil class occurs among the gas cells
        hasW, hasE, hasS, hasN = neighbour_flags(gas)
        assert not gas.all()
        for cls in (hasW & hasE & hasS & hasN, ~hasW & hasE, hasW & ~hasE, ~hasS & hasN, hasS & ~hasN):
            assert (gas & cls).any()
        inner = gas.copy()
        inner[[0, -1], :] = False
        inner[:, [0, -1]] = False
        assert (inner & ~(hasW & hasE & hasS & hasN)).any()   # one-sided next to the solid, not at the grid's edge only


def test_oracle_region_stride_and_subsets(hf):
    case = _sim(hf, "wedge", steps=2).case
    full = case.frame()
    f = case.frame(vars=("grad_p", "U"), region=(3, 40, 2, 21), stride=(5, 3))
    ii, jj = np.arange(3, 40, 5), np.arange(2, 21, 3)
    np.testing.assert_array_equal(f["i"], ii)
    np.testing.assert_array_equal(f["j"], jj)
    assert tuple(f["vars"]) == ("grad_p", "U") and f["values"].shape == (2, len(ii), len(jj))
    # gradients from the immediate neighbours, whatever the stride
    same_bits(f["values"][0], full["values"][V["grad_p"]][np.ix_(ii, jj)])
    same_bits(f["values"][1], full["values"][V["U"]][np.ix_(ii, jj)])
    np.testing.assert_array_equal(f["gas"], full["gas"][np.ix_(ii, jj)])
    np.testing.assert_array_equal(f["x"], full["x"][ii])
    one = case.frame(vars=["ducros"], region=(66, 67, 22, 23))
    same_bits(one["values"], full["values"][V["ducros"]][66:, 22:][None])


def _write(case, **fields):
    rec = np.frombuffer(case.records(), dtype=REC64).copy()
    for k, a in fields.items():
        if k == "rho":
            rec["S"][:, 0] = a.ravel()
        else:
            rec[k] = a.ravel()
    case.set_records(rec.tobytes())


def test_oracle_on_analytic_fields(hf):
    case = hf.Simulation(DECKS["wedge"](), "cpu").case
    gas = gas_of(case)
    hasW, hasE, hasS, hasN = neighbour_flags(gas)
    full = gas & (hasW | hasE) & (hasS | hasN)   # a neighbour in both directions: every gas cell of this deck
    assert (full == gas).all() and (gas & ~(hasW & hasE & hasS & hasN)).any() and gas.sum() > 1000
    x = (np.arange(case.nx) * case.dx)[:, None] + np.zeros((1, case.ny))
    y = (np.arange(case.ny) * case.dy)[None, :] + np.zeros((case.nx, 1))
    _write(case, rho=1.0 + 2.0 * x + 3.0 * y, U=-y, V=x)
    f = case.frame()["values"]
    np.testing.assert_allclose(f[V["grad_rho"]][full], np.sqrt(13.0), rtol=1e-9)
    np.testing.assert_allclose(f[V["vorticity"]][full], 2.0, rtol=1e-9)
    np.testing.assert_allclose(f[V["dilatation"]][full], 0.0, atol=1e-9)
    np.testing.assert_allclose(f[V["ducros"]][full], 0.0, atol=1e-18)
    _write(case, U=x, V=y)
    f = case.frame()["values"]
    np.testing.assert_allclose(f[V["dilatation"]][full], 2.0, rtol=1e-9)
    np.testing.assert_allclose(f[V["vorticity"]][full], 0.0, atol=1e-9)
    np.testing.assert_allclose(f[V["ducros"]][full], 1.0, rtol=1e-9)
    # a constant field: +0.0 in all five derived variables, everywhere
    one = np.ones((case.nx, case.ny))
    _write(case, rho=1.25 * one, U=3.0 * one, V=-2.0 * one, p=1.0e5 * one)
    f = case.frame()["values"]
    for var in FRAME_VARS[5:]:
        assert not f[V[var]].any() and not np.signbit(f[V[var]]).any(), var
    # non-gas cells read +0.0 in every variable
    assert not f[:, ~gas].any() and not np.signbit(f[:, ~gas]).any()


@functools.lru_cache(maxsize=None)
def _twin(name):
    """times [NSTEPS], frames [NSTEPS, 10, nx, ny] of a recorder-free run after each of its one-step calls."""
    import openhyperflow2d_amd as hf

    sim = _sim(hf, name)
    times, vals = [], []
    for _ in range(NSTEPS):
        sim.step(1)
        sim.solver.download()
        vals.append(np.asarray(sim.case.frame()["values"]).copy())
        times.append(sim.summary()["time"])
    out = np.array(times), np.array(vals)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(DECKS))
def test_recorder_equals_the_twin(hf, name):
    times, vals = _twin(name)
    sim = _sim(hf, name)
    sim.record_frames(vars=FRAME_VARS, capacity=64)
    h = sim.frame_history()
    assert h["total"] == 0 and h["values"].shape == (0, 10) + vals.shape[2:] and h["times"].shape == (0,)
    for n, res in [(1, False), (4, True), (7, False)]:
        sim.step(n, residual=res)
    h = sim.frame_history()
    assert h["total"] == 12 and h["values"].dtype == np.float64 and h["vars"] == FRAME_VARS
    same_bits(h["values"], vals[:12], name)
    np.testing.assert_array_equal(h["times"], times[:12])
    f = sim.case.frame()
    for k in STATIC:
        np.testing.assert_array_equal(h[k], f[k], err_msg=k)
    # recording moved nothing, and nothing compares constants
    sim.solver.download()
    same_bits(sim.case.frame()["values"], vals[11])
    assert (np.diff(times) > 0).all()
    for var in ("rho", "grad_rho", "grad_p", "vorticity", "dilatation", "ducros"):
        assert (vals[1:, V[var]] != vals[:-1, V[var]]).any(), var


def test_ring_wrap_region_stride_clear_and_rearm(hf):
    name = "wedge"
    times, vals = _twin(name)
    sim = _sim(hf, name)
    sim.record_frames(every=3, capacity=4)   # the default variables
    sim.step(NSTEPS)
    h = sim.frame_history()
    rows = list(range(2, NSTEPS, 3))   # steps 3, 6, ..., 24
    assert h["total"] == len(rows) == 8 and h["vars"] == ("rho", "grad_rho")
    same_bits(h["values"], vals[rows[-4:]][:, [V["rho"], V["grad_rho"]]])
    np.testing.assert_array_equal(h["times"], times[rows[-4:]])
    # a strided region on a second simulation, variables in the caller's order
    b = _sim(hf, name)
    b.record_frames(vars=("vorticity", "p", "ducros"), region=(1, 60, 0, 23), stride=(2, 3), capacity=3)
    b.step(5)
    hb = b.frame_history()
    ii, jj = np.arange(1, 60, 2), np.arange(0, 23, 3)
    np.testing.assert_array_equal(hb["i"], ii)
    np.testing.assert_array_equal(hb["j"], jj)
    assert hb["total"] == 5 and hb["values"].shape == (3, 3, len(ii), len(jj))
    for k, var in enumerate(("vorticity", "p", "ducros")):
        same_bits(hb["values"][:, k], vals[2:5, V[var]][:, ii][:, :, jj], var)
    # clear: the ring and the sampling count restart; the recorder stays armed
    b.clear_frames()
    z = b.frame_history()
    assert z["total"] == 0 and z["values"].shape == (0, 3, len(ii), len(jj))
    b.step(2)
    hb = b.frame_history()
    assert hb["total"] == 2
    same_bits(hb["values"][:, 1], vals[5:7, V["p"]][:, ii][:, :, jj])
    # arming again replaces the recorder
    b.record_frames(vars="T", every=2, capacity=8)
    b.step(4)
    hb = b.frame_history()
    assert hb["total"] == 2 and hb["vars"] == ("T",)
    same_bits(hb["values"][:, 0], vals[[8, 10], V["T"]])
    np.testing.assert_array_equal(hb["times"], times[[8, 10]])


def test_argument_errors_and_refusals(hf):
    sim = _sim(hf, "wedge")
    nx, ny = sim.case.nx, sim.case.ny
    bad = (dict(vars=()), dict(vars=("rho", "mach")), dict(vars=("rho", "p", "rho")), dict(region=(5, 5, 0, ny)),
           dict(region=(0, nx, 7, 3)), dict(region=(-1, nx, 0, ny)), dict(region=(0, nx + 1, 0, ny)),
           dict(region=(0, nx, 0, ny + 1)), dict(region=(0, nx, 0)), dict(stride=(0, 1)), dict(stride=(1, -2)),
           dict(every=0), dict(capacity=0), dict(vars=FRAME_VARS, capacity=2 ** 31 // (10 * nx * ny) + 1))
    for kw in bad:
        with pytest.raises(ValueError):
            sim.record_frames(**kw)
    for kw in bad[:11]:
        with pytest.raises(ValueError):
            sim.case.frame(**kw)
    with pytest.raises(RuntimeError):
        sim.frame_history()   # nothing armed: the refused calls left no recorder behind
    with pytest.raises(ValueError):
        sim.record_frames(vars=("rho",), region=(0, 1, 0, 1), capacity=2 ** 31 + 1)   # (2^31 itself is the bound)
    sim.record_frames(capacity=5, every=2)
    sim.step(4)
    before = sim.frame_history()
    for kw in bad:   # a refused call leaves the armed recorder as it was
        with pytest.raises(ValueError):
            sim.record_frames(**kw)
    after = sim.frame_history()
    assert before.keys() == after.keys() and after["total"] == 2
    for k in before:
        np.testing.assert_array_equal(before[k], after[k], err_msg=k)
    sim.step(2)
    assert sim.frame_history()["total"] == 3
    ref = hf.Simulation(DECKS["wedge"](), "ref")
    with pytest.raises(RuntimeError):
        ref.record_frames()


def test_a_strip_records_rows_and_refuses_gradients(hf):
    """One strip of several, built in-process without any collective: the row
    variables over the owned columns of the region, the gradient variables refused."""
    case = hf.Simulation(DECKS["wedge"](), "cpu").case
    for a, b in ((0, 30), (30, 67)):
        strip = hf.Simulation(DECKS["wedge"](), "cpu", gi0=a, gi1=b)
        strip.record_frames(vars=("rho", "U"), region=(4, 60, 0, 23), stride=(3, 1), capacity=2)
        h = strip.frame_history()
        want = [i for i in range(4, 60, 3) if a <= i < b]
        assert h["i"].tolist() == want and h["values"].shape == (0, 2, len(want), 23)
        np.testing.assert_array_equal(h["gas"], gas_of(case)[want])
        with pytest.raises(RuntimeError, match="strip"):
            strip.record_frames(vars=("rho", "grad_rho"))
        assert strip.frame_history()["vars"] == ("rho", "U")   # the armed recorder is intact


def test_cli_frames(hf, tmp_path):
    text = decks.step(37, 23, nmax=6, nout=3)
    for k, v in [("MonitorIndex", 1), ("ExitMonitorValue", 1e-30)]:
        text = decks.set_key(text, k, v)
    (tmp_path / "s.dat").write_text(text)
    out = tmp_path / "fr.npz"
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--cycles", "2", "--no-checkpoint",
            "--frames", str(out), "--frames-vars", "grad_rho,p,ducros", "--frames-every", "2", "--frames-capacity", "2",
            "--frames-stride", "2,3", timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert {"times", "values", "total", "vars", "i", "j", "x", "y", "gas"} == set(z.files)
    assert z["vars"].tolist() == ["grad_rho", "p", "ducros"]
    f = hf.Simulation(text, "cpu").case.frame(vars=("p",), stride=(2, 3))
    for k in ("i", "j", "x", "y", "gas"):
        np.testing.assert_array_equal(z[k], f[k], err_msg=k)
    assert z["values"].shape == (2, 3, 19, 8) and int(z["total"]) == 6
    assert (np.diff(z["times"]) > 0).all() and np.isfinite(z["values"]).all() and z["values"][:, 0].any()
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--frames", str(tmp_path / "no.npz"),
            "--frames-vars", "mach", timeout=120)
    assert r.returncode == 2 and "unknown variable" in r.stderr, r.stdout + r.stderr
    # a multi-rank launch is refused with a message, before anything runs
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--frames", str(tmp_path / "no.npz"),
            timeout=120, env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "one process" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "no.npz").exists()
