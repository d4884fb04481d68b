"""Every GPU step path reports Tg < 0 in the same call as the plain CPU stepper
(tables, protocol and comparison rules: tests/failure_cases.py; the CPU's own
conditions: test_failure_cases.py).

Ten kernel sites set the error word (the shared tile body, hf2d_lean_euler,
fill_body, hf2d_fused_euler, the hf2d_lns_step family, hf2d_lnm_step and
hf2d_lnm_hot); it reaches the host through the host_tail mirror of the tile
kernel's last workgroup or through hf2d_scalars_out, possibly across replayed
6-step graph windows.  Every test asserts which kernels ran (lean_tile_last,
lns_steps, lnm_steps, sk_mode, lns_ok), so a silent fall-back cannot pass.

Which natural failure reaches which site (found by removing one flag write at
a time from a scratch build; the cases that then fail): the shared tile body
-- every tile case; hf2d_lns_step -- step_cfl12, resonator, plate_sst and
sa_adiabatic; hf2d_lnm_step -- scramjet_cold; hf2d_lnm_hot -- scramjet (its
failing cell is a reacting one, and that kernel alone reports it)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from tests import failure_cases as fc
from tests import model_families as mf
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")


# --- the step paths -------------------------------------------------------------

class Path:
    """One step path: its smallest deck, the Simulation keywords and solver
    knobs that select it, and the facts that prove it ran."""

    def __init__(self, deck, kw=None, knobs=None, geom=None, tile=False, sk=mf.SK_GENERIC, lns_turb=None, lns_why=None,
                 lnm=False, lean_ok=None, sg=None):
        self.deck, self.kw, self.knobs, self.geom, self.tile = deck, kw or {}, knobs or {}, geom, tile
        self.sk, self.lns_turb, self.lns_why, self.lnm, self.lean_ok, self.sg = sk, lns_turb, lns_why, lnm, lean_ok, sg
        self.lns = lns_turb is not None

    def simulation(self, hf, cfl=None, keys=()):
        g = fc.simulation(hf, self.deck, "gpu", cfl, keys, **self.kw)
        sv = g.solver
        if self.geom:
            sv.cu_count = 0   # no two-cells-per-thread gate
            sv.lean_nt, sv.lean_cpt, sv.lean_tj = self.geom
        for k, v in self.knobs.items():
            setattr(sv, k, v)
        self.constructed(sv)
        return g

    def constructed(self, sv):
        """What construction must have found."""
        assert sv.sk_mode == self.sk, (sv.sk_mode, sv.sgl_why)
        if self.lean_ok is not None:
            assert sv.lean_ok == self.lean_ok, sv.lean_why
        if self.sg is not None:
            assert sv.lean_sg_ok == self.sg
        if self.lns:
            assert sv.lns_ok and sv.lns_turb == self.lns_turb and sv.lean_ns, (sv.lns_why, sv.lns_turb)
        elif self.lns_why is not None:
            assert (sv.lns_ok, sv.lns_why) == (False, self.lns_why)
        if self.lnm:
            assert sv.lnm_ok and sv.lean_mech, sv.lnm_why

    def ran(self, sv, lean_steps=True):
        """After a call of at least two steps from a lean state (or any call
        on a path without one): the kernels of the path ran, no others."""
        last = sv.lean_tile_last
        if self.tile:
            assert last["nt"] != 0, last
            if self.geom:
                assert (last["nt"], last["cpt"]) == self.geom[:2], last
        else:
            assert last["nt"] == 0, last
        if lean_steps:
            assert (sv.lns_steps > 0) == self.lns, sv.lns_steps
            assert (sv.lnm_steps > 0) == self.lnm, sv.lnm_steps


ADIABATIC_WHY = "wall heat transfer"
SK_MECH = 3   # (sk_mode of a deck in mechanism mode)
PATHS = {
    "tile_sg_256": Path("wedge", geom=fc.WEDGE_GEOMS[0], tile=True, lean_ok=True, sg=True),
    "tile_sg_64": Path("wedge", geom=fc.WEDGE_GEOMS[1], tile=True, lean_ok=True, sg=True),
    "tile_3gas": Path("triple_point", geom=fc.TRIPLE_GEOM, tile=True, lean_ok=True, sg=False),
    "lean_flat": Path("wedge", knobs=dict(lean_tile=False), lean_ok=True),            # hf2d_lean_euler
    "fused_euler": Path("wedge", kw=dict(lean=False)),                                # hf2d_fused_euler
    "split_generic": Path("wedge", kw=dict(lean=False, fused=False)),                 # hf2d_fill<SK_GENERIC>
    "split_sgt": Path("wedge_keps", sk=mf.SK_SGT, lns_why=ADIABATIC_WHY),             # hf2d_fill<SK_SGT>
    "split_sgl": Path("step", knobs=dict(lean_ns=False), sk=mf.SK_SGL),               # hf2d_fill<SK_SGL>
    "lns_laminar": Path("step", sk=mf.SK_SGL, lns_turb=2),   # (laminar: lns_turb keeps its default)
    "lns_keps": Path("resonator", sk=mf.SK_SGT, lns_turb=2),
    "lns_sst": Path("plate_sst", sk=mf.SK_SGT, lns_turb=3),
    "lns_sa": Path("sa_adiabatic", sk=mf.SK_SGT, lns_turb=4),
    "lean_mech": Path("scramjet", sk=SK_MECH, lnm=True),
}
# split_sgl switches lean_ns off after construction: what ran() must then see
PATHS["split_sgl"].lns = False


def _path_facts(pid, sv):
    p = PATHS[pid]
    if pid == "lean_flat":
        assert sv.lean and not sv.lean_tile
    if pid == "fused_euler":
        assert not sv.lean and sv.fused
    if pid == "split_generic":
        assert not sv.lean and not sv.fused
    if pid == "split_sgl":
        assert sv.lns_ok and not sv.lean_ns
    return p


def _poisoned(gpu, pid, cell, **knobs):
    """The path's simulation after step(3) and the poison."""
    g = PATHS[pid].simulation(gpu)
    _path_facts(pid, g.solver)
    for k, v in knobs.items():
        setattr(g.solver, k, v)
    g.step(fc.POISON_AFTER)
    g.solver.poison_cell(*cell)
    return g


def _cell(gpu, pid, which):
    deck = PATHS[pid].deck
    if which == "centre":
        return fc.centre_cell(deck)
    if isinstance(which, str):
        return fc.geometry_cells(gpu.native(), deck, PATHS[pid].geom)[which]
    return which


def _poison_cases():
    out = []
    for pid, p in PATHS.items():
        if p.deck in fc.POISON:
            cells = list(fc.POISON[p.deck].raises + fc.POISON[p.deck].quiet) + (list(fc.ROLES) if p.geom else [])
        else:
            cells = ["centre"]
        out += [(pid, c) for c in cells]
    return out


def _cid(v):
    return v if isinstance(v, str) else "%d_%d" % v


# --- a. poisoned, one step --------------------------------------------------------

@pytest.mark.parametrize("pid,which", _poison_cases(), ids=lambda v: _cid(v))
def test_poisoned_cell_reports_in_the_cpu_twins_step(gpu, pid, which):
    """step(3), poison, step(1): a report exactly when the CPU twin reports,
    ending `before iteration 4`; a cell that stays quiet stays quiet for 8 more
    single steps on both, and on the inviscid decks the gas cells, dt and time
    stay == the CPU's."""
    p = PATHS[pid]
    cell = _cell(gpu, pid, which)
    ref = fc.cpu_poison(p.deck, cell)
    g = _poisoned(gpu, pid, cell)
    sv = g.solver
    message = fc.step_raises(g)
    # (no lean N-S / mechanism step yet: steps 0 and 1 change is_init / is_mu_t, step 2 is the split
    # entry step, and the poison materialised the state, so step 3 is an entry step again)
    p.ran(sv, lean_steps=False)
    assert sv.lns_steps == 0 and sv.lnm_steps == 0
    print("%s %s: cpu %r, gpu %r" % (pid, cell, ref.message, message))
    assert (message is not None) == (ref.message is not None), (ref.message, message)
    if message is not None:
        assert message.endswith("before iteration %d" % (fc.POISON_AFTER + 1)), message
        return
    scalars = [(g.summary()["dt"], g.summary()["time"])]
    for _ in range(fc.QUIET_STEPS):
        assert fc.step_raises(g) is None
        scalars.append((g.summary()["dt"], g.summary()["time"]))
    p.ran(sv)
    if not fc.DECKS[p.deck].viscous:
        assert tuple(scalars) == ref.scalars
        bad = fc.misses_equal(g.field, g.summary(), ref.snap, ref.gas, fc.fields_of(p.deck))
        assert not bad, "\n".join(bad)


# --- b. poisoned, the flag carried to the end of a longer call ----------------------

def _first_raising_cell(gpu, pid):
    p = PATHS[pid]
    cell = fc.POISON[p.deck].raises[0] if p.deck in fc.POISON else fc.centre_cell(p.deck)
    assert fc.cpu_poison(p.deck, cell).message is not None
    return cell


@pytest.mark.parametrize("pid", list(PATHS))
def test_flag_survives_replayed_graph_windows(gpu, pid):
    """step(13) with step graphs after the poison: the failing step is a plain
    eager one (windows start at multiples of 6 steps), a 6-step graph window
    follows it, and the report comes at the end of the call with the call's
    last iteration.  The fault-free twin shows that a window was launched."""
    p = PATHS[pid]
    twin = p.simulation(gpu)
    twin.solver.use_graph = True
    twin.step(fc.POISON_AFTER)
    twin.step(13)
    assert twin.solver.graph_launches > 0, (twin.solver.graph_launches, twin.solver.graph_captures)
    assert twin.solver.use_graph   # (a failed capture switches graphs off)
    p.ran(twin.solver)
    g = _poisoned(gpu, pid, _first_raising_cell(gpu, pid), use_graph=True)
    message = fc.step_raises(g, 13)
    assert g.solver.graph_launches > 0 and g.solver.use_graph
    assert message is not None and message.endswith("before iteration %d" % (fc.POISON_AFTER + 13)), message


@pytest.mark.parametrize("pid", list(PATHS))
def test_flag_survives_eager_steps_without_the_host_mirror(gpu, pid):
    """step(5) eager with host_tail off: the word set by the first step is
    read four steps later by hf2d_scalars_out."""
    g = _poisoned(gpu, pid, _first_raising_cell(gpu, pid), use_graph=False, host_tail=False)
    message = fc.step_raises(g, 5)
    assert g.solver.graph_launches == 0
    PATHS[pid].ran(g.solver)
    assert message is not None and message.endswith("before iteration %d" % (fc.POISON_AFTER + 5)), message


# --- c. natural failures ---------------------------------------------------------

INVISCID_NATURAL = ["tile_sg_256", "tile_sg_64", "lean_flat", "fused_euler", "split_generic"]


def _graph_call_raises(gpu, p, n):
    """Once more as one call of iteration + 7 steps with step graphs."""
    g = p.simulation(gpu, n.cfl, n.keys)
    g.solver.use_graph = True
    steps = n.iteration + 7
    message = fc.step_raises(g, steps)
    assert message is not None, "no report from one call of %d steps" % steps
    # (a call that crosses the deck's Nmax reports at the cycle roll, before its last step)
    if steps <= g.case.nmax:
        assert message.endswith("before iteration %d" % steps), message
        assert g.solver.use_graph   # (a failed capture switches graphs off)
        if steps >= 13:   # (the first window starts at step 6 and the call's last step is eager)
            assert g.solver.graph_launches > 0


@pytest.mark.parametrize("pid", INVISCID_NATURAL)
def test_natural_failure_inviscid(gpu, pid):
    """The wedge at CFL 1.5, nothing poisoned, in calls of step(1) with no
    download in between (the tile kernel fails from its own lean state): the
    report comes in the CPU's call, dt and time before it == the CPU's, and
    the fields of the state it is made from == the CPU's."""
    p, n = PATHS[pid], fc.NATURAL_BY_ID["wedge"]
    ref = fc.cpu_natural(n.id)
    g = p.simulation(gpu, n.cfl, n.keys)
    sv = g.solver
    lasts = []
    done, message, scalars = fc.march_until_report(g, n.iteration + fc.AFTER,
                                                   lambda k, msg: lasts.append(dict(sv.lean_tile_last)))
    print("%s: cpu iteration %r, gpu %r (%r)" % (pid, ref.iteration, done, message))
    assert done == ref.iteration == n.iteration, (done, ref.iteration, message)
    assert message.endswith("before iteration %d" % (done + 1)), message
    assert tuple(scalars) == ref.scalars
    # the kernel of the failing call: every call but the first (the flat entry step) is a tile step
    if p.tile:
        assert lasts[0]["nt"] == 0 and all((q["nt"], q["cpt"]) == p.geom[:2] for q in lasts[1:]), lasts
    else:
        assert all(q["nt"] == 0 for q in lasts), lasts
    # the state before the report, from a twin that runs up to it in one call
    b = p.simulation(gpu, n.cfl, n.keys)
    b.step(n.iteration)
    p.ran(b.solver)
    bad = fc.misses_equal(b.field, b.summary(), ref.snap, ref.gas, fc.fields_of(n.deck))
    assert not bad, "\n".join(bad)
    _graph_call_raises(gpu, p, n)


# (natural case, lean path or None, what switches the lean kernels off for the split twin)
VISCOUS_NATURAL = [
    ("step", "lns_laminar", "lean_ns"),
    ("step_cfl12", "lns_laminar", "lean_ns"),
    ("resonator", "lns_keps", "lean_ns"),
    ("plate_sst", "lns_sst", "lean_ns"),
    ("sa_adiabatic", "lns_sa", "lean_ns"),
    ("scramjet", "lean_mech", "lean_mech"),
    ("scramjet_cold", "lean_mech", "lean_mech"),
    ("sa", None, None),
    ("wall_law", None, None),
]
# iterations of the lean paths' first lean step: step 0 resets the turbulence (is_init), step 1 changes
# is_mu_t, step 2 is the split entry step; a report at an earlier iteration comes from a split kernel
FIRST_LEAN_ITERATION = 3
SPLIT_ONLY = {"sa": Path("sa", sk=mf.SK_SGT, lns_why=ADIABATIC_WHY),
              "wall_law": Path("wall_law", sk=mf.SK_SGT, lns_why=ADIABATIC_WHY)}


@pytest.mark.parametrize("nid,pid,knob", VISCOUS_NATURAL, ids=[v[0] for v in VISCOUS_NATURAL])
def test_natural_failure_viscous(gpu, nid, pid, knob):
    """Viscous and mechanism decks, nothing poisoned, in calls of step(1) with
    no download in between: the lean kernels report in the call of their split
    twin (lean_ns / lean_mech off: bitwise the same run by the existing tests)
    and of the CPU; the lean step counter has grown before the failing call
    and in it; the state the report is made from obeys the 1e-9 rule.

    The step deck at CFL 1.5 reports in its third step, the split entry step
    of the lean kernels (steps 0 and 1 change is_init / is_mu_t and run the
    split kernels): there the counter must still be 0, and step_cfl12 is the
    laminar case that fails from the lean state.  The scramjet's failing cell
    reacts: hf2d_lnm_hot reports it; scramjet_cold (no cell reacts) is
    hf2d_lnm_step's."""
    n = fc.NATURAL_BY_ID[nid]
    ref = fc.cpu_natural(nid)
    p = PATHS[pid] if pid else SPLIT_ONLY[nid]
    assert p.deck == n.deck
    g = p.simulation(gpu, n.cfl, n.keys)
    sv = g.solver
    counts = []
    done, message, scalars = fc.march_until_report(g, n.iteration + fc.AFTER,
                                                   lambda k, msg: counts.append(sv.lns_steps + sv.lnm_steps))
    print("%s: cpu iteration %r, gpu %r (%r), lean steps after every call %r" % (nid, ref.iteration, done, message, counts))
    assert done == ref.iteration == n.iteration, (done, ref.iteration, message)
    assert message.endswith("before iteration %d" % (done + 1)), message
    assert sv.lean_tile_last["nt"] == 0
    if pid and n.iteration >= FIRST_LEAN_ITERATION:
        assert (sv.lns_steps > 0, sv.lnm_steps > 0) == (p.lns, p.lnm)
        # grown before the failing call, and the failing call itself was a lean step
        assert counts[-2] > 0 and counts[-1] == counts[-2] + 1, counts
    else:
        assert counts[-1] == 0, counts   # every step so far was a split one
    for k, ((dt, t), (dt_c, t_c)) in enumerate(zip(scalars, ref.scalars)):
        assert abs(dt - dt_c) <= fc.REL * dt_c and abs(t - t_c) <= fc.REL * t_c, (k, dt, dt_c, t, t_c)
    if pid:
        # the split twin
        s = p.simulation(gpu, n.cfl, n.keys)
        setattr(s.solver, knob, False)
        done_s, message_s, scalars_s = fc.march_until_report(s, n.iteration + fc.AFTER)
        assert s.solver.lns_steps == 0 and s.solver.lnm_steps == 0
        assert done_s == done, (done_s, done, message_s)
        assert scalars_s == scalars   # (dt and time of the lean kernels == the split kernels')
    # the state before the report, from a twin that runs up to it in one call
    b = p.simulation(gpu, n.cfl, n.keys)
    b.step(n.iteration)
    figs, bad = fc.misses_close(b.field, b.summary(), ref.snap, ref.gas, fc.fields_of(n.deck))
    print("%s before the report: %s" % (nid, " ".join("%s=%.2e" % kv for kv in figs.items())))
    assert not bad, "\n".join(bad)
    _graph_call_raises(gpu, p, n)


# --- d. sticky and clearable -------------------------------------------------------

@pytest.mark.parametrize("pid", ["tile_sg_256", "tile_sg_64", "tile_3gas"])
def test_report_is_sticky_until_an_upload(gpu, pid):
    """After a report a further step(1) reports again (as on the CPU twin,
    marched the same way first); upload() of records downloaded before the
    poison clears the word: 13 steps run and every field is finite."""
    p = PATHS[pid]
    cell = fc.POISON[p.deck].raises[0]
    c = fc.cpu(p.deck)
    c.step(3)
    c.step(3)
    c.solver.poison_cell(*cell)
    assert fc.step_raises(c) is not None and fc.step_raises(c) is not None

    g = p.simulation(gpu)
    sv = g.solver
    g.step(3)
    good = g.records()   # (a download: the next call starts with the flat entry step)
    g.step(3)
    p.ran(sv)
    sv.poison_cell(*cell)
    first = fc.step_raises(g)
    p.ran(sv)
    again = fc.step_raises(g)
    p.ran(sv)
    assert first is not None and first.endswith("before iteration 7"), first
    assert again is not None and again.endswith("before iteration 8"), again
    g.case.set_records(good)
    sv.upload()
    assert fc.step_raises(g, 13) is None
    p.ran(sv)
    gas = g.field("solid") == 0.0
    for f in fc.fields_of(p.deck):
        assert np.isfinite(g.field(f)[gas]).all(), f
    s = g.summary()
    assert np.isfinite(s["dt"]) and s["dt"] > 0 and np.isfinite(s["time"])


def test_fresh_simulation_after_a_failed_one_equals_cpu(gpu):
    """A failed solver leaves nothing behind in the process: the next
    Simulation steps == the CPU stepper."""
    p = PATHS["tile_sg_256"]
    cell = fc.POISON[p.deck].raises[0]
    g = _poisoned(gpu, "tile_sg_256", cell)
    assert fc.step_raises(g, 2) is not None
    p.ran(g.solver)
    fresh = p.simulation(gpu)
    c = fc.cpu(p.deck)
    for n in (4, 9):
        fresh.step(n)
        c.step(n)
        p.ran(fresh.solver)
        bad = fc.misses_equal(fresh.field, fresh.summary(), fc.snapshot(c, fc.fields_of(p.deck)), c.field("solid") == 0.0,
                              fc.fields_of(p.deck))
        assert not bad, "\n".join(bad)


# --- e. autotune ---------------------------------------------------------------------

def test_autotune_survives_an_unstable_transient(gpu, monkeypatch):
    """ThreadBlockSize = 0 with the search on, on the wedge that reports at
    iteration 6: the trial steps report, autotune() stops (`stopped:` in the
    log), restores the start, and the run itself then fails in the CPU's
    call from the CPU's state."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "1")
    n = fc.NATURAL_BY_ID["wedge"]
    text = decks.set_key(fc.deck_text(n.deck, n.cfl), "ThreadBlockSize", 0)
    ref = fc.cpu_natural(n.id)
    g = gpu.Simulation(text, "gpu")     # must not raise
    assert g.solver.autotune_enabled and g.case.thread_block_size == 0
    print(g.autotune_log)
    assert "stopped:" in g.autotune_log and fc.MESSAGE in g.autotune_log, g.autotune_log
    assert g.summary()["iteration"] == 0 and g.solver.lns_steps == 0 and g.solver.graph_launches == 0
    done, message, scalars = fc.march_until_report(g, n.iteration + fc.AFTER)
    assert done == ref.iteration, (done, message)
    assert message.endswith("before iteration %d" % (done + 1)), message
    assert tuple(scalars) == ref.scalars
    assert g.solver.lean_tile_last["nt"] != 0, g.solver.lean_tile_last
    b = gpu.Simulation(text, "gpu")
    assert "stopped:" in b.autotune_log
    b.step(n.iteration)
    bad = fc.misses_equal(b.field, b.summary(), ref.snap, ref.gas, fc.fields_of(n.deck))
    assert not bad, "\n".join(bad)


# --- 3. the driver's failure path ------------------------------------------------------

STEM = "Wedge15_80x30"


def _driver_deck():
    text = decks.wedge15(80, 30, nmax=20, nout=5)
    text = decks.set_key(text, "MonitorIndex", 1)           # residual exit monitor ...
    return decks.set_key(text, "ExitMonitorValue", 1e-30)   # ... never met: run every requested cycle


def _failed_run(hf, backend, d, fault, lean=None):
    d.mkdir()
    sim = hf.Simulation(_driver_deck(), backend, workdir=str(d), lean=(backend == "gpu") if lean is None else lean)
    with pytest.raises(RuntimeError) as ei:
        sim.run(max_cycles=3, outdir=str(d), verbose=True, fault=fault)
    return sim, str(ei.value)


def _report_lines(msg):
    """The `Tg=... in cell (i, j)` line and the `CT:` line after it."""
    lines = msg.splitlines()
    k = [q for q, s in enumerate(lines) if s.startswith("Tg=") and " in cell (" in s]
    assert len(k) == 1, msg
    assert lines[k[0] + 1].strip().startswith("CT:"), msg
    return lines[k[0]], lines[k[0] + 1]


@pytest.mark.parametrize("lean", [False, True], ids=["fused_euler", "lean_tile"])
def test_driver_fault_at_an_output_step_matches_cpu(gpu, tmp_path, lean):
    """fault = step:25, an output step: the GPU synchronises right after the
    poisoned step, as the CPU does.  Both download the state one step after
    the poison: the error snapshot, the report's cell and the surviving
    checkpoint are the CPU's, byte for byte.

    lean=False (hf2d_fused_euler) against the plain CPU stepper.  The lean tile
    kernel (the default) against the CPU's lean stepper: the poison changes
    rhoE alone and leaves the record's stored fluxes as they were, which the
    plain stepper goes on using for one step while the lean steppers recompute
    them from the poisoned state, so one step after the poison the two CPU
    steppers -- otherwise bit for bit the same (test_steppers.py) -- differ
    themselves (test_failure_cases.py pins that), and the GPU's lean run
    reported Tg = -1.43146e+25 in cell (40, 14) where the plain CPU stepper
    reports -1.4267e+25 in (39, 15).  The checkpoint, written before the
    poison, is the plain CPU stepper's in both cases."""
    import json

    g, mg = _failed_run(gpu, "gpu", tmp_path / "g", "step:25", lean)
    c, mc = _failed_run(gpu, "cpu", tmp_path / "c", "step:25", lean)
    if lean:
        _failed_run(gpu, "cpu", tmp_path / "p", "step:25", False)   # the plain CPU stepper's checkpoint
    assert g.solver.lean_ok and c.solver.lean_ok and g.solver.lean == c.solver.lean == lean
    assert (g.solver.lean_tile_last["nt"] != 0) == lean, g.solver.lean_tile_last
    for m in (mg, mc):
        assert "unstability" in m and "Error snapshot" in m and "last good checkpoint (iteration 20)" in m, m
    assert "before iteration 26" in mg and "on iteration 25," in mc
    print(_report_lines(mg), _report_lines(mc))
    assert _report_lines(mg) == _report_lines(mc)
    twin = {STEM + "-err.plt": "c", STEM + ".hf2d": "c" if not lean else "p"}
    for name, d in twin.items():
        a, b = (tmp_path / "g" / name).read_bytes(), (tmp_path / d / name).read_bytes()
        assert len(a) > 0 and a == b, name
    for d in ("g", "c"):
        assert json.loads((tmp_path / d / (STEM + ".hf2d.meta")).read_text())["iteration"] == 20


def test_driver_fault_between_output_steps_and_recovery(gpu, tmp_path):
    """fault = step:27: the report comes at the next output step (`before
    iteration 31`), the snapshot names a gas cell whose Tg is not >= 0, and
    the checkpoint is that of a fault-free run stopped after cycle 1.  A new
    Simulation on that checkpoint then runs one more cycle == a CPU
    simulation resumed from the same file."""
    import json
    import re

    g, mg = _failed_run(gpu, "gpu", tmp_path / "g", "step:27")
    assert "unstability" in mg and "before iteration 31" in mg, mg
    assert "Error snapshot" in mg and "last good checkpoint (iteration 20)" in mg, mg
    err = tmp_path / "g" / (STEM + "-err.plt")
    assert err.exists() and err.stat().st_size > 0
    line, ct = _report_lines(mg)
    m = re.match(r"Tg=(\S+) in cell \((\d+), (\d+)\) of rank 0", line)
    assert m, line
    tg, i, j = float(m.group(1)), int(m.group(2)), int(m.group(3))
    assert not tg >= 0
    assert "CT_NODE_IS_SET_2D" in ct and "CT_SOLID_2D" not in ct, ct
    assert g.field("solid")[i, j] == 0.0 and not g.field("T")[i, j] >= 0
    assert json.loads((tmp_path / "g" / (STEM + ".hf2d.meta")).read_text())["iteration"] == 20

    (tmp_path / "ok").mkdir()
    ok = gpu.Simulation(_driver_deck(), "gpu", workdir=str(tmp_path / "ok"))
    assert ok.run(max_cycles=1, outdir=str(tmp_path / "ok"), verbose=False)[0] == 1
    ckpt = (tmp_path / "g" / (STEM + ".hf2d")).read_bytes()
    assert len(ckpt) > 0 and ckpt == (tmp_path / "ok" / (STEM + ".hf2d")).read_bytes()

    # recovery
    r = gpu.Simulation(_driver_deck(), "gpu", workdir=str(tmp_path / "g"), use_checkpoint=True)
    c = gpu.Simulation(_driver_deck(), "cpu", workdir=str(tmp_path / "g"), use_checkpoint=True, lean=False)
    (tmp_path / "out").mkdir()
    for s in (r, c):
        assert s.summary()["iteration"] == 20
        assert s.run(max_cycles=1, outdir=str(tmp_path / "out"), outputs=False, checkpoint=False, verbose=False)[0] == 1
        assert s.summary()["iteration"] == 40
    assert r.solver.lean_tile_last["nt"] != 0
    gas = c.field("solid") == 0.0
    bad = fc.misses_equal(r.field, r.summary(), fc.snapshot(c, fc.EULER_FIELDS), gas, fc.EULER_FIELDS)
    assert not bad, "\n".join(bad)
    assert all(np.isfinite(r.field(f)[gas]).all() for f in fc.EULER_FIELDS)


def test_cli_gpu_fault_exit_code(gpu, tmp_path):
    """python -m openhyperflow2d_amd run --backend gpu --fault-inject step:7
    in a child process: exit code 3, the report on stderr, the snapshot on disk."""
    (tmp_path / "w.dat").write_text(_driver_deck())
    env = dict(os.environ, PYTHONPATH=ROOT, HF2D_AUTOTUNE="0")
    r = subprocess.run([sys.executable, "-m", "openhyperflow2d_amd", "run", "w.dat", "--backend", "gpu", "--cycles", "2",
                        "--fault-inject", "step:7"], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-2000:]
    assert "unstability" in r.stderr and "backend=gpu" in r.stdout
    assert (tmp_path / (STEM + "-err.plt")).exists()
