"""Per-step probe recorder (Simulation.record_probes / probe_history) on the
CPU backend, which samples its own arrays after every step.

The oracle is a twin simulation of the same backend and settings without a
recorder, advanced with step(1) and read with field() and summary()["time"]
after every step; every comparison is bitwise.  Both start from
tests.perturb.perturb, so no cell equals its neighbours."""
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


def _text():
    return decks.wedge15(40, 12, **BIG)


def _sim(hf):
    s = hf.Simulation(_text(), "cpu")
    perturb(s, SEED)
    return s


def _gas_cells(sim, n):
    """n non-solid cells spread over the grid (first / last column included)."""
    solid = sim.field("solid")
    nx, ny = solid.shape
    cells = []
    for i in np.linspace(0, nx - 1, n).astype(int):
        j = int(np.flatnonzero(solid[i] == 0.0)[-1 if len(cells) % 2 else 0])
        cells.append((int(i), j))
    return cells


def twin_rows(sim, cells, schedule):
    """Advance the recorder-free twin one step at a time over the schedule's
    calls; returns (times [n], rows [n, len(cells), 5]) read from field()."""
    times, rows = [], []
    for n, res in schedule:
        for k in range(n):
            sim.step(1, residual=res and k == n - 1)
            sim.solver.download()
            f = [np.asarray(sim.case.field(v)) for v in PROBE_VARS]
            rows.append([[a[i, j] for a in f] for i, j in cells])
            times.append(sim.summary()["time"])
    return np.array(times), np.array(rows)


def test_vars_order_is_documented():
    assert PROBE_VARS == ("p", "T", "rho", "U", "V")


def test_history_equals_the_twin(hf):
    a, b = _sim(hf), _sim(hf)
    cells = _gas_cells(a, 3)
    a.record_probes(cells, capacity=64)
    for n, res in SCHEDULE:
        a.step(n, residual=res)
    h = a.probe_history()
    t, rows = twin_rows(b, cells, SCHEDULE)
    assert NSTEPS == 14 and h["total"] == 14
    assert h["values"].shape == (14, 3, 5) and h["times"].shape == (14,)
    assert h["owned"].tolist() == [True, True, True]
    np.testing.assert_array_equal(h["values"], rows)
    np.testing.assert_array_equal(h["times"], t)
    assert len({tuple(r) for r in rows[-1]}) == 3 and not (rows[0] == rows[-1]).all()   # probes and steps differ
    # recording leaves the run unchanged
    for f in PROBE_VARS + ("k", "R", "CP"):
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)
    assert a.summary()["dt"] == b.summary()["dt"]


def test_ring_keeps_the_last_rows(hf):
    a, b = _sim(hf), _sim(hf)
    cells = _gas_cells(a, 3)
    a.record_probes(cells, capacity=5)
    for n, res in SCHEDULE:
        a.step(n, residual=res)
    h = a.probe_history()
    t, rows = twin_rows(b, cells, SCHEDULE)
    assert h["total"] == 14 and h["values"].shape == (5, 3, 5)
    np.testing.assert_array_equal(h["values"], rows[-5:])
    np.testing.assert_array_equal(h["times"], t[-5:])


def test_rearming_and_clearing_restart_the_count(hf):
    a, b = _sim(hf), _sim(hf)
    cells = _gas_cells(a, 3)
    a.record_probes(cells, capacity=8)
    a.step(4)
    assert a.probe_history()["total"] == 4
    a.record_probes(cells[:2], capacity=8)
    assert a.probe_history()["total"] == 0 and a.probe_history()["values"].shape == (0, 2, 5)
    a.step(3)
    h = a.probe_history()
    t, rows = twin_rows(b, cells[:2], [(7, False)])
    assert h["total"] == 3
    np.testing.assert_array_equal(h["values"], rows[4:])
    np.testing.assert_array_equal(h["times"], t[4:])
    a.clear_probe_history()
    assert a.probe_history()["total"] == 0
    a.step(1)
    assert a.probe_history()["total"] == 1


def test_refusals(hf):
    a = _sim(hf)
    solid = a.field("solid")
    nx, ny = solid.shape
    si, sj = (int(v[0]) for v in np.nonzero(solid))
    gas = _gas_cells(a, 1)[0]
    for cells, cap in [([], 8), ([(nx, 0)], 8), ([(0, ny)], 8), ([(-1, 0)], 8), ([(si, sj)], 8), ([gas], 0),
                       ([gas] * 65, 8)]:
        with pytest.raises(ValueError):
            a.record_probes(cells, capacity=cap)
    with pytest.raises(RuntimeError):
        a.probe_history()   # nothing armed: the refused calls left no recorder behind
    a.record_probes([gas] * 64, capacity=1)
    a.step(2)
    assert a.probe_history()["values"].shape == (1, 64, 5)
    ref = hf.Simulation(_text(), "ref")
    with pytest.raises(RuntimeError):
        ref.record_probes([gas])


def _py(*args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", *args], capture_output=True, text=True,
                          env=env, **kw)


def test_cli_probe_history(hf, tmp_path):
    text = decks.wedge15(40, 12, nmax=6, nout=3)
    case = hf.native().Case.from_deck(text, ".", False)
    text = decks.set_key(text, "NumMonitorPoints", 2)
    text = decks.set_key(decks.set_key(text, "MonitorIndex", 1), "ExitMonitorValue", 1e-30)
    pts = [(0.3 * 40 * case.dx, 0.8 * 12 * case.dy), (0.9 * 40 * case.dx, 0.85 * 12 * case.dy)]
    for q, (x, y) in enumerate(pts):
        text = decks.set_key(text, "Point-%d.X" % (q + 1), x)
        text = decks.set_key(text, "Point-%d.Y" % (q + 1), y)
    (tmp_path / "w.dat").write_text(text)
    out = tmp_path / "hist.npz"
    r = _py("run", str(tmp_path / "w.dat"), "--backend", "cpu", "--cycles", "2", "--no-checkpoint",
            "--probe-history", str(out), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert {"times", "values", "cells", "vars"} <= set(z.files)
    assert z["vars"].tolist() == list(PROBE_VARS)
    assert z["cells"].tolist() == [[int(x / case.dx), int(y / case.dy)] for x, y in pts]
    assert z["values"].shape == (12, 2, 5) and z["times"].shape == (12,)
    assert (np.diff(z["times"]) > 0).all() and np.isfinite(z["values"]).all()
    mon = [f for f in tmp_path.iterdir() if f.name.startswith("Monitors-")]
    assert mon, "the Monitors file is still written"
    # a multi-rank launch is refused with a message, before anything runs
    r = subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", "run", str(tmp_path / "w.dat"), "--backend", "cpu",
                        "--probe-history", str(tmp_path / "no.npz")], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PYTHONPATH=ROOT, WORLD_SIZE="2", RANK="0"))
    assert r.returncode == 2 and "one process" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "no.npz").exists()
