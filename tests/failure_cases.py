"""The instability report (Tg < 0) on every step path: the case tables and the
protocol (a plain module, no fixtures; CPU conditions: test_failure_cases.py,
GPU against CPU: test_gpu_failure_paths.py).

A cell whose recovered temperature is negative (mechanism mode: not above
MECH_TMIN) sets an error word; the host raises `Computational unstability
(Tg < 0)` at its next read of it.  The plain per-cell CPU stepper,
Simulation(text, "cpu", lean=False), raises inside the failing step and names
the iteration it was about to complete ("on iteration N", N steps done); the
GPU raises at the end of the step() call that holds that step and names the
call's last iteration ("before iteration M", M steps counted).

Poisoned cells.  step(3), solver.poison_cell(i, j) (rhoE = -1e30), step(1).
POISON lists, per deck, the cells that raise in that step on the CPU and those
that do not raise in it nor in 8 more steps (measured on the CPU stepper;
test_failure_cases.py asserts the table).  geometry_cells() adds the cells a
tile geometry makes special; what they do is whatever the CPU twin does
(cpu_poison()), never a table.

Natural failures.  Nothing is poisoned: the deck runs at CFL = 1.5 with a
constant CFL_Scenario (cfl()), or is one of two reference decks that blow up
as they stand.  NATURAL pins the iteration of the CPU's report.  The step deck
at CFL 1.5 reports in its third step, which on the GPU is still the split
entry step of the lean N-S kernels (the first two steps change is_init /
is_mu_t); "step_cfl12" is the same deck at CFL 1.2, which lasts until
iteration 11 and so fails from the lean state.  The scramjet's failing cell is
a reacting one: on the GPU's lean mechanism path the kernel that re-evaluates
the reacting cells after their kinetics (hf2d_lnm_hot) reports it.
"scramjet_cold" is the same deck with ChemTmin = 1e6 K, so that no cell
reacts and the tile kernel (hf2d_lnm_step) evaluates, and reports, every cell.
"""
import collections
import functools
import os

import numpy as np

from tests import model_families as mf
from tests.perturb import FIELDS as EULER_FIELDS
from tests.perturb import perturb

NS_FIELDS = mf.NS_FIELDS
REL = mf.REL
BIG = dict(nmax=10 ** 6, nout=10 ** 5)
MESSAGE = "Tg < 0"
QUIET_STEPS = 8          # single steps a cell that does not raise is marched on
POISON_AFTER = 3         # steps before the poison

Deck = collections.namedtuple("Deck", "build workdir perturb viscous")


def _ref(name, keys=()):
    def build():
        from openhyperflow2d_amd.models import decks

        with open(os.path.join(mf.REF, name, "deck.dat"), "r", errors="replace") as f:
            text = f.read()
        for k, v in keys:
            text = decks.set_key(text, k, v)
        return text

    return build


def _gen(name, *a, keys=(), **kw):
    def build():
        from openhyperflow2d_amd.models import decks

        text = getattr(decks, name)(*a, **dict(BIG, **kw))
        for k, v in keys:
            text = decks.set_key(text, k, v)
        return text

    return build


ADIABATIC = (("isAdiabaticWall", 1),)
SA_START = dict(seed=1, amp=0.05)   # (model_families.py: with amp 0.05 the deck reaches Tg < 0 at iteration 24)

DECKS = {
    "wedge": Deck(_gen("wedge15", 221, 41), ".", None, False),
    "triple_point": Deck(_gen("triple_point", 160, 51), ".", None, False),
    "scramjet": Deck(_gen("scramjet", 37, 23), ".", None, True),
    "wedge_keps": Deck(_gen("wedge15", 200, 60, navier_stokes=True, turbulence=4), ".", None, True),
    "step": Deck(_gen("step", 240, 80), ".", None, True),
    "resonator": Deck(_gen("resonator", 300, 40), ".", None, True),
    "plate_sst": Deck(_gen("flat_plate", 200, 60, turbulence=6, keys=ADIABATIC), ".", None, True),
    "wall_law": Deck(_ref("wall_law"), os.path.join(mf.REF, "wall_law"), None, True),
    "sa": Deck(_ref("spalart_allmaras_blowup"), os.path.join(mf.REF, "spalart_allmaras_blowup"), SA_START, True),
    "sa_adiabatic": Deck(_ref("spalart_allmaras_blowup", ADIABATIC), os.path.join(mf.REF, "spalart_allmaras_blowup"),
                         SA_START, True),
}


def cfl(text, value=1.5):
    """The deck at a constant CFL number."""
    from openhyperflow2d_amd.models import decks

    text = decks.set_key(text, "CFL", float(value))
    return decks.set_table(text, "CFL_Scenario", [(0.0, float(value)), (1.0e9, float(value))])


@functools.lru_cache(maxsize=None)
def deck_text(deck, cfl_value=None, keys=()):
    from openhyperflow2d_amd.models import decks

    text = DECKS[deck].build()
    for k, v in keys:
        text = decks.set_key(text, k, v)
    return text if cfl_value is None else cfl(text, cfl_value)


def simulation(hf, deck, backend, cfl_value=None, keys=(), **kw):
    """The deck on `backend`, perturbed where the deck's row says so."""
    d = DECKS[deck]
    sim = hf.Simulation(deck_text(deck, cfl_value, tuple(keys)), backend, workdir=d.workdir, **kw)
    if d.perturb:
        perturb(sim, **d.perturb)
    return sim


def cpu(deck, cfl_value=None, keys=()):
    import openhyperflow2d_amd as hf

    return simulation(hf, deck, "cpu", cfl_value, keys, lean=False)


def fields_of(deck):
    return NS_FIELDS if DECKS[deck].viscous else EULER_FIELDS


def step_raises(sim, n=1, **kw):
    """step(n): None, or the message of the RuntimeError it raised (which
    must be the instability report)."""
    try:
        sim.step(n, **kw)
    except RuntimeError as e:
        assert MESSAGE in str(e), str(e)
        return str(e)
    return None


# --- poisoned cells -----------------------------------------------------------

Poison = collections.namedtuple("Poison", "raises quiet")
POISON = {
    # (220, 20) and (191, 8) are solid
    "wedge": Poison(((110, 20), (0, 20), (110, 0), (110, 40), (15, 15), (16, 16), (220, 40), (0, 0)),
                    ((220, 20), (191, 8))),
    "triple_point": Poison(((80, 25), (0, 0), (159, 50)), ()),
    "scramjet": Poison(((18, 11), (30, 5)), ()),
}
# (threads per tile workgroup, cells per thread, tile height override) of tests/perturb.GEOMS
WEDGE_GEOMS = ((256, 1, 0), (64, 2, 8))
TRIPLE_GEOM = (256, 1, 0)
ROLES = ("tile_first", "tile_last", "partial_tile", "last_row")


def geometry_cells(native, deck, geom):
    """{role: (i, j)} for the deck's grid under the tile geometry (nt, cpt,
    tj): the first cell of a tile of the upper tile row, the last cell of a
    tile of the first tile row (both of the middle tile column), a cell of
    the partial last tile column and a cell of the grid's last row."""
    nx, ny = grid(deck)
    nt, cpt, tj = geom
    T = native.lean_tile_geom(nx, ny, nt, tj, cpt)
    TI, TJ, nbi, nbj = T["TI"], T["TJ"], T["nbi"], T["nbj"]
    assert nbi >= 3 and nbj >= 2 and nx % TI != 0, T
    bi = nbi // 2
    last = (nbi - 1) * TI
    return {"tile_first": (bi * TI, (nbj - 1) * TJ), "tile_last": (bi * TI + TI - 1, TJ - 1),
            "partial_tile": (last + (nx - last) // 2, ny - 3), "last_row": (nx // 3, ny - 1)}


@functools.lru_cache(maxsize=None)
def grid(deck):
    import re

    text = deck_text(deck)
    return tuple(int(re.search(r"<data/%s=\s*(\d+)" % k, text).group(1)) for k in ("MaxX", "MaxY"))


def centre_cell(deck):
    """The gas cell nearest the grid's centre (Chebyshev distance; ties: the
    first in (i, j) order): the poisoned cell of the decks POISON does not list."""
    solid = np.asarray(cpu(deck).field("solid"))
    nx, ny = solid.shape
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    d = np.maximum(np.abs(i - nx // 2), np.abs(j - ny // 2)).astype(float)
    d[solid != 0.0] = np.inf
    q = int(np.argmin(d))
    return q // ny, q % ny


def snapshot(sim, fields):
    return mf.snapshot(sim, fields)


PoisonRef = collections.namedtuple("PoisonRef", "message scalars snap gas")


@functools.lru_cache(maxsize=None)
def cpu_poison(deck, cell):
    """The CPU twin: step(3), poison, step(1); where that does not raise,
    QUIET_STEPS more single steps.  message: the report of the first step that
    raised, or None; scalars: (dt, time) after every step that did not; snap:
    the fields after the last of them (computed once, shared, never modified)."""
    c = cpu(deck)
    c.step(POISON_AFTER)
    c.solver.poison_cell(*cell)
    scalars, message = [], None
    for _ in range(1 + QUIET_STEPS):
        message = step_raises(c)
        if message is not None:
            break
        s = c.summary()
        scalars.append((s["dt"], s["time"]))
    gas = c.field("solid") == 0.0
    gas.setflags(write=False)
    return PoisonRef(message, tuple(scalars), snapshot(c, fields_of(deck)) if message is None else None, gas)


# --- natural failures ---------------------------------------------------------

# iteration: the N of the CPU's "on iteration N" (N steps completed, the report comes from step N + 1)
Natural = collections.namedtuple("Natural", "id deck cfl iteration keys", defaults=((),))
NATURAL = [
    Natural("wedge", "wedge", 1.5, 6),
    Natural("scramjet", "scramjet", 1.5, 4),
    Natural("scramjet_cold", "scramjet", 1.5, 4, (("ChemTmin", 1.0e6),)),
    Natural("step", "step", 1.5, 2),
    Natural("step_cfl12", "step", 1.2, 11),
    Natural("plate_sst", "plate_sst", 1.5, 9),
    Natural("resonator", "resonator", 1.5, 5),
    Natural("wall_law", "wall_law", None, 3),
    Natural("sa", "sa", None, 24),
    Natural("sa_adiabatic", "sa_adiabatic", None, 24),
]
NATURAL_BY_ID = {n.id: n for n in NATURAL}
AFTER = 3     # calls marched past the pinned iteration before a test gives up

NaturalRef = collections.namedtuple("NaturalRef", "iteration message scalars snap gas")


@functools.lru_cache(maxsize=None)
def cpu_natural(nid):
    """The CPU twin marched in calls of step(1) until it reports (at most
    iteration + AFTER calls).  iteration: steps completed before the report
    (None: no report); scalars: (dt, time) after every completed step; snap:
    the fields after the last completed step."""
    n = NATURAL_BY_ID[nid]
    c = cpu(n.deck, n.cfl, n.keys)
    scalars, message, snap = [], None, None
    for _ in range(n.iteration + AFTER):
        if len(scalars) == n.iteration:   # (the state the report is made from)
            snap = snapshot(c, fields_of(n.deck))
        message = step_raises(c)
        if message is not None:
            break
        s = c.summary()
        scalars.append((s["dt"], s["time"]))
    gas = c.field("solid") == 0.0
    gas.setflags(write=False)
    return NaturalRef(len(scalars) if message is not None else None, message, tuple(scalars), snap, gas)


def march_until_report(sim, calls, after_call=None):
    """Calls of step(1) on sim, at most `calls`, with no download in between
    (a download materialises the lean state, and the next step would be the
    split entry step).  Returns (steps completed before the report or None,
    the message, (dt, time) after every completed call)."""
    scalars = []
    for _ in range(calls):
        message = step_raises(sim)
        if after_call is not None:
            after_call(len(scalars), message)
        if message is not None:
            return len(scalars), message, scalars
        s = sim.summary()
        scalars.append((s["dt"], s["time"]))
    return None, None, scalars


# --- comparison -----------------------------------------------------------------

def misses_equal(field, summary, snap, gas, fields):
    """dt, time and the gas cells of `fields` bit for bit; one line per miss."""
    bad = ["%s: %r != %r" % (q, summary[q], snap[q]) for q in ("dt", "time") if summary[q] != snap[q]]
    for f in fields:
        x, y = field(f)[gas], snap[f][gas]
        if not np.array_equal(x, y):
            bad.append("%s: %d gas cells differ" % (f, int((x != y).sum())))
    return bad


def misses_close(field, summary, snap, gas, fields):
    """The project's 1e-9 rule (model_families.py): per field max |x - cpu|
    over gas <= REL * max |cpu| over gas, dt and time to REL relative; a
    field the CPU leaves NaN somewhere must be NaN in the same cells and is
    compared on the others.  Returns ({field: relative difference}, misses)."""
    out, bad = {}, []
    for q in ("dt", "time"):
        if not abs(summary[q] - snap[q]) <= REL * abs(snap[q]):
            bad.append("%s: %r against %r" % (q, summary[q], snap[q]))
    for f in fields:
        x, y = field(f), snap[f]
        if not (np.isnan(x) == np.isnan(y))[gas].all():
            bad.append(f + ": NaN on other cells than the CPU's")
        cells = gas & ~np.isnan(y)
        if not cells.any():
            continue
        top, d = float(np.abs(y[cells]).max()), float(np.abs(x - y)[cells].max())
        out[f] = d / top if top > 0 else d
        if not d <= REL * top:   # (a NaN misses)
            bad.append("%s: max |diff| %.3e > %.1e * %.6e (rel %.3e)" % (f, d, REL, top, out[f]))
    return out, bad
