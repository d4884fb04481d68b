"""The turbulence-model families and contour / source decks of tests/fixtures/ref
across a cycle boundary: the case table and the protocol (a plain module, no
fixtures; CPU conditions: test_model_family_decks.py, GPU against CPU:
test_gpu_model_families.py).

Protocol.  The deck is tests/fixtures/ref/<deck>/deck.dat with the row's keys
set through decks.set_key, read with its directory as workdir (tsagi_airfoil
names a side file).  Both simulations start from perturb(sim, seed=1,
amp=0.02) -- with the default 0.05 spalart_allmaras_blowup reaches Tg < 0 at
iteration 24 on the CPU -- and march

    run(1, tmp, outputs=False, checkpoint=False, verbose=False)
    step(4, residual=True); step(6, residual=False); step(3, residual=True)

The run() call marches the deck's own Nmax steps (30; wall_law_plate 60,
zeldovich_reacting 20) and then cycle_update(): y+ from the wall friction
velocity.  Chien's k-eps and van Driest's mixing length damp with y+, which is
0 until then: both keep one value of mu_t over the whole field through the
first cycle and only the steps after it exercise their model code and the y+
kernels.  The reference is the plain per-cell CPU stepper,
Simulation(text, "cpu", lean=False); every call is compared.

Comparison rules (gas = every cell that is not solid; no other cell is left
out):

  "equal"  dt and time ==, assert_array_equal on EULER_FIELDS: the bar
           test_gpu_tile_shapes.py holds the inviscid kernels to.
  "1e-9"   per field max |gpu - cpu| over gas <= 1e-9 * max |cpu| over gas,
           dt and time to 1e-9 relative: the project's bound for GPU against
           CPU on the viscous paths (device and host libm differ in the last
           place of exp / pow / tanh).  Viscous rows compare NS_FIELDS.

GPU paths (test_gpu_model_families.py asserts which kernels ran):

  "default"  whatever DeviceSolver picks.  Viscous rows: the single-gas
             turbulent split kernels hf2d_predict / hf2d_fill<SK_SGT> (every
             viscous deck here has isAdiabaticWall = 0, which rules the lean
             N-S tiles out and runs hf2d_wall_solid / hf2d_wall_wall).
             Inviscid rows: the lean tile kernels, or, where the row names a
             lean_why, the fused Euler kernel.
  "generic"  hf2d_fill<SK_GENERIC> (viscous: sgl = lean_ns = False; inviscid:
             lean = fused = False, the split predict / fill pair).
  "lns"      LNS rows only: the deck with isAdiabaticWall = 1, on the lean
             N-S tiles, through lns_materialize() at the cycle boundary and
             the lean re-entry after it.

Left out: wall_law (stops with Tg < 0 at iteration 3 by design: test_gpu_failure_paths.py);
restart_from_hf2d (resumes from a checkpoint, no cold start to perturb);
wedge_keps_wallheat, step_euler, oblique_shock, wedge15_200x40_euler and
wedge15_200x60_ns_keps (large, and test_gpu_kernels.py already marches them).

No row needed a bound above 1e-9 (largest difference measured on an MI355X,
relative to the field's max: 1.1e-11, S7 of keps_chien; every algebraic
model, Smagorinsky, both Spalart-Allmaras decks and zeldovich_reacting: 0),
so no row carries a CPU sensitivity figure D."""
import collections
import functools
import os
import tempfile

import numpy as np

from tests.perturb import FIELDS as EULER_FIELDS
from tests.perturb import flat_fraction, perturb

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fixtures", "ref")
NS_FIELDS = EULER_FIELDS + ["mu", "lam", "mu_t", "y_plus", "S7", "S8"]
SEED, AMP = 1, 0.02
AFTER_RUN = [(4, True), (6, False), (3, True)]   # the step() calls that follow the run() call
REL = 1e-9

SK_GENERIC, SK_SGL, SK_SGT = 0, 1, 2

# mu_t: "varied"  at least 1000 distinct values on the gas cells at the end;
#       "const"   the reference's own behaviour keeps a handful of values
#                 (mu_t / mu ~ 5): GPU == CPU exactly;
#       None      inviscid.
# y_damped: mu_t has one value until the first cycle_update() and is varied after it.
# nan: fields the reference itself leaves NaN on gas cells (the fixture's
#      _hf2d_nan_canonical hash pins them); the NaN cells must be the same
#      on the GPU and every other cell is compared as usual.
# lean_why: inviscid rows; "" = lean-eligible (tile kernels by default).
Row = collections.namedtuple("Row", "id deck keys viscous model mu_t y_damped nan rule paths lean_why lns_turb lns_why")


def _ns(deck, model, mu_t="varied", y_damped=False, nan=()):
    return Row(deck, deck, (), True, model, mu_t, y_damped, tuple(nan), "1e-9", ("default", "generic"), None, None, None)


def _eu(deck, model, keys=(), rule="equal", lean_why="", id=None):
    return Row(id or deck, deck, tuple(keys), False, model, None, False, (), rule, ("default", "generic"), lean_why, None,
               None)


def _lns(deck, model, lns_turb, lns_why="", y_damped=False):
    return Row("lns:" + deck, deck, (("isAdiabaticWall", 1),), True, model, "varied", y_damped, (), "1e-9", ("lns",), None,
               lns_turb, lns_why)


VISCOUS = [
    _ns("prandtl", "Prandtl mixing length (TurbExtModel 0)"),
    _ns("van_driest", "van Driest damping exp(-y+ / 26) (1)", y_damped=True),
    _ns("escudier", "Escudier length cap (2)"),
    _ns("klebanoff", "Klebanoff intermittency (3)"),
    # the integral model only writes Re_local: mu_t stays at the reset value 5 mu (1 value)
    _ns("integral_model", "integral model", mu_t="const"),
    _ns("keps_chien", "Chien k-eps, f_mu = 1 - exp(-0.0115 y+) (5)", y_damped=True),
    _ns("keps_jones_launder", "Jones-Launder k-eps (6)"),
    _ns("keps_launder_sharma", "Launder-Sharma k-eps (7)"),
    _ns("keps_rng", "RNG k-eps (8)"),
    _ns("smagorinsky", "Smagorinsky"),
    # TurbStartIter = 100: the model never starts inside the schedule, mu_t keeps 3
    # values (0 on the walls, 5 mu, 5 mu / 1000), and the reference's S-A source is
    # 0 / 0 wherever nu~ = 0: S7 is NaN on 3716 of the 3959 gas cells from the first
    # cycle on (measured on the CPU stepper)
    _ns("spalart_allmaras_start", "Spalart-Allmaras before TurbStartIter", mu_t="const", nan=("S7",)),
    _ns("spalart_allmaras_blowup", "Spalart-Allmaras (10)"),
    _ns("axisym_keps", "standard k-eps, axisymmetric (FlowType 1)"),
    _ns("naca_airfoil_ns", "standard k-eps round the NACA contour"),
    _ns("wall_law_plate", "standard k-eps with wall-law nodes, Nmax 60"),
    _ns("monitors_heatflux_cx", "standard k-eps with monitor points and the Cx contour"),
]

INVISCID = [
    _eu("axisym_euler", "Euler, axisymmetric (FlowType 1)"),
    _eu("bff_linear", "blending factor function 0"),
    _eu("bff_linear", "blending factor function 1", keys=(("BFF", 1),), id="bff_linear:BFF=1"),
    _eu("bff_linear", "blending factor function 2", keys=(("BFF", 2),), id="bff_linear:BFF=2"),
    _eu("bff_square_relax", "blending factor function 3"),
    _eu("bff_sqrt_relax", "blending factor function 5"),
    _eu("circle", "circle contour"),
    _eu("solid_rect", "solid rectangle contour"),
    _eu("naca_airfoil", "NACA airfoil contour"),
    _eu("tsagi_airfoil", "TsAGI airfoil contour from a side file"),
    _eu("gas_source", "gas source (volume sources: not lean-eligible)", lean_why="gas sources"),
    # the Zeldovich rate is A exp(-Ta / T) pow(c_fu, a) pow(c_ox, b) (physics.hpp): device
    # exp / pow differ from the host's in the last place, so this row takes the viscous
    # rule on the inviscid field list; 12 x 12 cells, Nmax 20, isAdiabaticWall = 0
    _eu("zeldovich_reacting", "Zeldovich one-step chemistry", rule="1e-9", lean_why="wall heat transfer"),
]

LNS = [
    _lns("keps_jones_launder", "Jones-Launder k-eps on the lean N-S tiles", 2),
    _lns("keps_launder_sharma", "Launder-Sharma k-eps on the lean N-S tiles", 2),
    _lns("keps_rng", "RNG k-eps on the lean N-S tiles", 2),
    _lns("spalart_allmaras_blowup", "Spalart-Allmaras on the lean N-S tiles", 4),
    # Chien's model reads the previous level's p: the lean N-S tiles must refuse it
    _lns("keps_chien", "Chien k-eps: refused by the lean N-S tiles, split SK_SGT kernels", 2, lns_why="Chien k-eps",
         y_damped=True),
]

ROWS = VISCOUS + INVISCID + LNS
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)


def fields_of(row):
    return NS_FIELDS if row.viscous else EULER_FIELDS


def deck_text(row):
    from openhyperflow2d_amd.models import decks

    with open(os.path.join(REF, row.deck, "deck.dat"), "r", errors="replace") as f:
        text = f.read()
    for k, v in row.keys:
        text = decks.set_key(text, k, v)
    return text


def simulation(hf, row, backend, **kw):
    """The row's deck on `backend`, perturbed."""
    sim = hf.Simulation(deck_text(row), backend, workdir=os.path.join(REF, row.deck), **kw)
    perturb(sim, seed=SEED, amp=AMP)
    return sim


def march(sim, tmp):
    """The schedule; yields the call's index after every call."""
    sim.run(1, str(tmp), outputs=False, checkpoint=False, verbose=False)
    yield 0
    for q, (n, res) in enumerate(AFTER_RUN):
        sim.step(n, residual=res)
        yield q + 1


def snapshot(sim, fields):
    s = sim.summary()
    snap = {"dt": s["dt"], "time": s["time"], "iteration": s["iteration"]}
    for f in fields:
        a = sim.field(f).copy()
        a.setflags(write=False)
        snap[f] = a
    return snap


Reference = collections.namedtuple("Reference", "snaps gas flat_start flat_end")


def _cpu_march(row):
    import openhyperflow2d_amd as hf

    c = simulation(hf, row, "cpu", lean=False)
    flat0 = flat_fraction(c)
    gas = c.field("solid") == 0.0
    gas.setflags(write=False)
    with tempfile.TemporaryDirectory() as tmp:
        snaps = tuple(snapshot(c, fields_of(row)) for _ in march(c, tmp))
        assert os.listdir(tmp) == []
    return Reference(snaps, gas, flat0, flat_fraction(c))


@functools.lru_cache(maxsize=None)
def cpu_reference(row_id):
    """Snapshots of the generic CPU stepper after every call of the schedule
    (computed once per row, shared, never modified)."""
    return _cpu_march(BY_ID[row_id])


def distinct(a, gas):
    return int(np.unique(a[gas]).size)


def misses(row, field, summary, snap, gas):
    """field(name) / summary of the simulation under test against one CPU
    snapshot, by the row's rule.  Returns ({field: difference relative to the
    field's max}, [one line per quantity that misses the rule])."""
    out, bad = {}, []
    if row.rule == "equal":
        for q in ("dt", "time"):
            if summary[q] != snap[q]:
                bad.append("%s: %r != %r" % (q, summary[q], snap[q]))
        for f in fields_of(row):
            x, y = field(f)[gas], snap[f][gas]
            out[f] = float(np.abs(x - y).max()) / max(float(np.abs(y).max()), 1e-300)
            if not np.array_equal(x, y):   # (the CPU's fields are finite: a NaN differs)
                bad.append("%s: %d cells differ, rel %.3e" % (f, int((x != y).sum()), out[f]))
        return out, bad
    assert row.rule == "1e-9", row.rule
    for q in ("dt", "time"):
        if not abs(summary[q] - snap[q]) <= REL * abs(snap[q]):
            bad.append("%s: %r against %r" % (q, summary[q], snap[q]))
    for f in fields_of(row):
        x, y = field(f), snap[f]
        cells = gas
        if f in row.nan:
            if not (np.isnan(x) == np.isnan(y))[gas].all():
                bad.append(f + ": NaN on other cells than the CPU's")
            cells = gas & ~np.isnan(y)
        top = float(np.abs(y[cells]).max())
        d = float(np.abs(x - y)[cells].max())
        out[f] = d / top if top > 0 else d
        if row.mu_t == "const" and f == "mu_t" and not np.array_equal(x[gas], y[gas]):
            bad.append("mu_t: %d cells differ where the rule is ==" % int((x != y)[gas].sum()))
        if not d <= REL * top:   # (a NaN misses)
            bad.append("%s: max |diff| %.3e > %.1e * %.6e (rel %.3e)" % (f, d, REL, top, out[f]))
    return out, bad


def compare(row, field, summary, snap, gas):
    """misses(), as an assertion; returns the figures."""
    out, bad = misses(row, field, summary, snap, gas)
    assert not bad, "; ".join(bad)
    return out
