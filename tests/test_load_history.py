"""Per-step load recorder (Simulation.record_loads / load_history) on the CPU
backend, which evaluates the shared plan (core/load_plan.hpp) on its own
arrays after every step.

The oracle is the host integrals themselves: after every step of the armed
run the records are downloaded and Case.force_parts / x_force / y_force /
mass_flow_x are read; every comparison is bitwise.  All runs start from
tests.perturb.perturb, so no wall cell equals its neighbour."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import LOAD_PARTS
from tests.conftest import ROOT
from tests.perturb import perturb

SEED = 1
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
REF = os.path.join(ROOT, "tests", "fixtures", "ref")

DECKS = {
    "wedge_67x23": lambda: decks.wedge15(67, 23, **BIG),
    "wedge_40x7": lambda: decks.wedge15(40, 7, **BIG),
    "step": lambda: decks.step(37, 23, **BIG),
    "resonator": lambda: decks.resonator(37, 23, **BIG),
    "scramjet": lambda: decks.scramjet(37, 23, **BIG),
    "triple_point": lambda: decks.triple_point(160, 51, **BIG),
}
# decks of tests/fixtures/ref with walls: a body in the stream, wall-law nodes, an axisymmetric N-S case
REF_DECKS = ["solid_rect", "naca_airfoil_ns", "wall_law_plate", "axisym_keps", "monitors_heatflux_cx"]


def targets(case):
    """The boxes and cuts of the issue's protocol for a grid of nx x ny cells."""
    nx, ny, dx, dy = case.nx, case.ny, case.dx, case.dy
    L, H = nx * dx, ny * dy
    solid = np.asarray(case.field("solid"))
    boxes = [(0.0, 0.0, 2 * L, 2 * H), (0.25 * L, 0.1 * H, 0.5 * L, 0.6 * H), empty_box(case, solid)]
    cuts = [((nx // 2 + 0.5) * dx, 0.0, 2 * H), ((nx // 2 + 0.5) * dx, 0.3 * H, 0.4 * H), (0.5 * dx, 0.0, 2 * H),
            ((nx - 0.5) * dx, 0.0, 2 * H), ((nx + 3) * dx, 0.0, 2 * H)]
    return boxes, cuts


def empty_box(case, solid):
    """A one-cell box that holds no wall node (its four force lists are empty)."""
    nx, ny = solid.shape
    for i in range(nx // 2, nx):
        for j in range(ny // 2, ny):
            if case.force_parts((i + 0.5) * case.dx, (j + 0.5) * case.dy, 0.0, 0.0)[5:] == (0, 0, 0, 0):
                return ((i + 0.5) * case.dx, (j + 0.5) * case.dy, 0.0, 0.0)
    raise AssertionError("no wall-free cell")


def host_loads(case, boxes, cuts):
    """(forces [nboxes, 4], counts [nboxes, 4], span [nboxes], totals [nboxes, 2], mass_flow [ncuts]) of the records."""
    parts = [case.force_parts(*b) for b in boxes]
    forces = np.array([p[:4] for p in parts]).reshape(len(boxes), 4)
    counts = np.array([p[5:] for p in parts], dtype=np.int64).reshape(len(boxes), 4)
    span = np.array([p[4] for p in parts])
    totals = np.array([[case.x_force(*b), case.y_force(*b)] for b in boxes]).reshape(len(boxes), 2)
    mf = np.array([case.mass_flow_x(*c) for c in cuts])
    return forces, counts, span, totals, mf


def cut_counts(case, cuts):
    """Cells of each cut as mass_flow_rate_x walks them: the non-solid cells of column int(x0 / dx), rows
    [int(y0 / dy), int((y0 + dy) / dy)) inside the grid (none when the column is outside it)."""
    solid = np.asarray(case.field("solid"))
    nx, ny = solid.shape
    out = []
    for x0, y0, dy in cuts:
        i, j0, j1 = int(x0 / case.dx), int(y0 / case.dy), int((y0 + dy) / case.dy)
        out.append(int((solid[i, j0:min(j1, ny)] == 0.0).sum()) if i < nx else 0)
    return np.array(out, dtype=np.int64)


def check_against_host(sim, boxes, cuts, calls):
    """Arm, then after every step: download, compare the newest row with the host integrals."""
    sim.record_loads(boxes, cuts, capacity=64)
    rows = []
    for n, res in calls:
        for k in range(n):
            sim.step(1, residual=res and k == n - 1)
            sim.solver.download()
            forces, counts, span, totals, mf = host_loads(sim.case, boxes, cuts)
            h = sim.load_history()
            assert h["total"] == len(rows) + 1 and h["forces"].shape == (len(rows) + 1, len(boxes), 4)
            np.testing.assert_array_equal(h["forces"][-1], forces)
            np.testing.assert_array_equal(h["forces"][-1, :, 0] + h["forces"][-1, :, 1], totals[:, 0])
            np.testing.assert_array_equal(h["forces"][-1, :, 2] + h["forces"][-1, :, 3], totals[:, 1])
            np.testing.assert_array_equal(h["mass_flow"][-1], mf)
            np.testing.assert_array_equal(h["terms"]["box_terms"], counts)
            np.testing.assert_array_equal(h["terms"]["cut_terms"], cut_counts(sim.case, cuts))
            np.testing.assert_array_equal(h["span"], span)
            assert h["times"][-1] == sim.summary()["time"]
            rows.append((forces, mf))
    return sim.load_history(), rows


def test_parts_order_is_documented():
    assert LOAD_PARTS == ("Fx_p", "Fx_d", "Fy_p", "Fy_d")


@pytest.mark.parametrize("name", list(DECKS))
def test_history_equals_the_host_integrals(hf, name):
    sim = hf.Simulation(DECKS[name](), "cpu")
    perturb(sim, SEED)
    boxes, cuts = targets(sim.case)
    h, rows = check_against_host(sim, boxes, cuts, [(1, False), (3, True), (1, False)])
    bt, ct = h["terms"]["box_terms"], h["terms"]["cut_terms"]
    assert (bt[2] == 0).all() and ct[4] == 0 and ct[0] > 1   # the wall-free box, the cut beyond the grid
    assert (h["forces"][:, 2] == 0).all() and not np.signbit(h["forces"][:, 2]).any()   # empty lists read +0.0
    assert (h["mass_flow"][:, 4] == 0).all() and not np.signbit(h["mass_flow"][:, 4]).any()
    assert ct[1] < ct[0]
    # non-vacuity: five distinct values over the five steps wherever there are terms
    # (the last column takes more than one value: the resonator's closed end starts at rest)
    for c, distinct in ((0, 5), (1, 5), (3, 2)):
        assert len(set(h["mass_flow"][:, c].tolist())) >= distinct, (name, c)
    if name == "triple_point":
        assert (bt == 0).all()   # no wall node: every force list is empty
    else:
        assert bt[0].max() > 0
        for b in (0, 1):
            total = h["forces"][:, b, 0] + h["forces"][:, b, 1] + h["forces"][:, b, 2] + h["forces"][:, b, 3]
            assert len(set(total.tolist())) == 5, (name, b)
    assert (np.diff(h["times"]) > 0).all()


@pytest.mark.parametrize("deck", REF_DECKS)
def test_reference_decks_with_walls(hf, deck):
    with open(os.path.join(REF, deck, "deck.dat"), "r", errors="replace") as f:
        text = f.read()
    sim = hf.Simulation(text, "cpu", workdir=os.path.join(REF, deck))
    perturb(sim, SEED, amp=0.02)
    boxes, cuts = targets(sim.case)
    h, _ = check_against_host(sim, boxes, cuts, [(2, False), (1, True)])
    assert h["terms"]["box_terms"][0].max() > 0, "the deck has wall terms"


def test_upload_rebuilds_the_plan(hf):
    """New records with other flags under an armed recorder: the lists follow them."""
    sim = hf.Simulation(DECKS["step"](), "cpu")
    perturb(sim, SEED)
    boxes, cuts = targets(sim.case)
    sim.record_loads(boxes, cuts, capacity=8)
    sim.step(1)
    perturb(sim, SEED + 1)   # (set_records + upload)
    sim.step(1)
    sim.solver.download()
    forces, counts, _, _, mf = host_loads(sim.case, boxes, cuts)
    h = sim.load_history()
    assert h["total"] == 2
    np.testing.assert_array_equal(h["forces"][-1], forces)
    np.testing.assert_array_equal(h["mass_flow"][-1], mf)


def test_ring_clear_and_rearming(hf):
    a = hf.Simulation(DECKS["step"](), "cpu")
    perturb(a, SEED)
    boxes, cuts = targets(a.case)
    full, _ = check_against_host(a, boxes, cuts, [(9, False)])
    b = hf.Simulation(DECKS["step"](), "cpu")
    perturb(b, SEED)
    b.record_loads(boxes, cuts, capacity=4)
    b.step(9)
    h = b.load_history()
    assert h["total"] == 9 and h["forces"].shape == (4, 3, 4) and h["mass_flow"].shape == (4, 5)
    np.testing.assert_array_equal(h["forces"], full["forces"][-4:])
    np.testing.assert_array_equal(h["mass_flow"], full["mass_flow"][-4:])
    np.testing.assert_array_equal(h["times"], full["times"][-4:])
    b.clear_load_history()
    h = b.load_history()
    assert h["total"] == 0 and h["forces"].shape == (0, 3, 4) and h["times"].shape == (0,)
    b.step(1)
    assert b.load_history()["total"] == 1
    # arming again replaces the ring: other lists, the count restarts
    b.record_loads(boxes[:1], (), capacity=4)
    h = b.load_history()
    assert h["total"] == 0 and h["forces"].shape == (0, 1, 4) and h["mass_flow"].shape == (0, 0)
    b.record_loads((), cuts[:2], capacity=4)
    b.step(2)
    h = b.load_history()
    assert h["total"] == 2 and h["forces"].shape == (2, 0, 4) and h["mass_flow"].shape == (2, 2)


def test_refusals(hf):
    sim = hf.Simulation(DECKS["wedge_40x7"](), "cpu")
    box, cut = (0.0, 0.0, 1.0, 1.0), (0.01, 0.0, 1.0)
    bad = [((), (), 8), ([box] * 17, (), 8), ((), [cut] * 17, 8), ([box], [cut], 0),
           ([(0.0, float("nan"), 1.0, 1.0)], (), 8), ((), [(float("inf"), 0.0, 1.0)], 8), ([(0.0, 0.0, 1.0)], (), 8),
           ((), [box], 8)]
    for boxes, cuts, cap in bad:
        with pytest.raises(ValueError):
            sim.record_loads(boxes, cuts, capacity=cap)
    with pytest.raises(RuntimeError):
        sim.load_history()   # nothing armed: the refused calls left no recorder behind
    sim.record_loads([box] * 16, [cut] * 16, capacity=1)
    sim.step(2)
    h = sim.load_history()
    assert h["forces"].shape == (1, 16, 4) and h["mass_flow"].shape == (1, 16) and h["total"] == 2
    ref = hf.Simulation(DECKS["wedge_40x7"](), "ref")
    with pytest.raises(RuntimeError):
        ref.record_loads([box], [cut])


def test_a_refused_rearm_leaves_the_recorder_whole(hf):
    """Cuts armed, a re-arm with boxes refused: the armed lists, the ring's shape and its rows stay, also
    across an upload() that rebuilds the plan."""
    sim = hf.Simulation(DECKS["step"](), "cpu")
    perturb(sim, SEED)
    boxes, cuts = targets(sim.case)
    sim.record_loads((), cuts[:2], capacity=8)
    sim.step(2)
    with pytest.raises(ValueError):
        sim.record_loads(boxes + [(0.0, float("nan"), 1.0, 1.0)], cuts, capacity=8)
    with pytest.raises(ValueError):
        sim.record_loads(boxes, cuts, capacity=0)
    perturb(sim, SEED + 1)   # (set_records + upload: the plan is rebuilt)
    sim.step(1)
    sim.solver.download()
    h = sim.load_history()
    assert h["total"] == 3 and h["forces"].shape == (3, 0, 4) and h["mass_flow"].shape == (3, 2)
    np.testing.assert_array_equal(h["mass_flow"][-1], [sim.case.mass_flow_x(*c) for c in cuts[:2]])
    np.testing.assert_array_equal(h["terms"]["cut_terms"], cut_counts(sim.case, cuts[:2]))


def test_a_strip_solver_refuses(hf):
    """One strip of several, built in-process without any collective."""
    strip = hf.Simulation(DECKS["wedge_67x23"](), "cpu", gi0=0, gi1=30)
    with pytest.raises(RuntimeError, match="strip"):
        strip.record_loads([(0.0, 0.0, 1.0, 1.0)], ())
    strip = hf.Simulation(DECKS["wedge_67x23"](), "cpu", gi0=30, gi1=67)
    with pytest.raises(RuntimeError, match="strip"):
        strip.record_loads((), [(0.01, 0.0, 1.0)])


def _py(*args, **kw):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.update(kw.pop("env", {}))
    return subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", *args], capture_output=True, text=True,
                          env=env, **kw)


def test_cli_load_history(hf, tmp_path):
    text = decks.step(37, 23, nmax=6, nout=3)
    case = hf.native().Case.from_deck(text, ".", False)
    L, H = case.nx * case.dx, case.ny * case.dy
    for k, v in [("MonitorIndex", 1), ("ExitMonitorValue", 1e-30), ("is_Cx_calc", 1), ("x_body", 0.0), ("y_body", 0.0), ("dx_body", L), ("dy_body", H),
                 ("Cx_Flow_Index", 1), ("NumXCut", 2), ("CutX-1.x0", 0.5 * L), ("CutX-1.y0", 0.0), ("CutX-1.dy", H),
                 ("CutX-2.x0", 0.9 * L), ("CutX-2.y0", 0.25 * H), ("CutX-2.dy", 0.5 * H)]:
        text = decks.set_key(text, k, v)
    case = hf.native().Case.from_deck(text, ".", False)
    boxes, cuts = case.load_targets
    assert len(boxes) == 1 and len(cuts) == 2
    (tmp_path / "s.dat").write_text(text)
    out = tmp_path / "loads.npz"
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--cycles", "2", "--no-checkpoint",
            "--load-history", str(out), timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    z = np.load(out)
    assert {"times", "forces", "mass_flow", "box_terms", "cut_terms", "span", "total", "boxes", "cuts",
            "parts"} <= set(z.files)
    assert z["parts"].tolist() == list(LOAD_PARTS)
    assert z["boxes"].tolist() == [list(b) for b in boxes] and z["cuts"].tolist() == [list(c) for c in cuts]
    assert z["forces"].shape == (12, len(boxes), 4) and z["mass_flow"].shape == (12, len(cuts))
    assert z["times"].shape == (12,) and (np.diff(z["times"]) > 0).all() and int(z["total"]) == 12
    assert np.isfinite(z["forces"]).all() and np.isfinite(z["mass_flow"]).all()
    # a multi-rank launch is refused with a message, before anything runs
    r = _py("run", str(tmp_path / "s.dat"), "--backend", "cpu", "--load-history", str(tmp_path / "no.npz"),
            timeout=120, env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 2 and "one process" in r.stderr, r.stdout + r.stderr
    assert not (tmp_path / "no.npz").exists()
