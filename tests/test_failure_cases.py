"""The CPU conditions of tests/failure_cases.py: the plain per-cell CPU stepper
reports Tg < 0 exactly where the tables say, so that the GPU tests
(test_gpu_failure_paths.py), which take their expectations from the CPU twin,
cannot pass because nothing ever fails."""
import numpy as np
import pytest

from tests import failure_cases as fc


@pytest.mark.parametrize("deck", list(fc.POISON))
def test_poisoned_cells_raise_or_stay_quiet_as_tabulated(hf, deck):
    """step(3), poison, step(1): every cell of `raises` reports in that step
    ("on iteration 3": three steps were completed); every cell of `quiet`
    marches 1 + 8 steps without a report and leaves finite gas cells."""
    row = fc.POISON[deck]
    assert not set(row.raises) & set(row.quiet)
    for cell in row.raises:
        ref = fc.cpu_poison(deck, cell)
        assert ref.message is not None, cell
        assert "Computational unstability (Tg < 0) on iteration %d," % fc.POISON_AFTER in ref.message, (cell, ref.message)
        assert ref.scalars == ()
    for cell in row.quiet:
        ref = fc.cpu_poison(deck, cell)
        assert ref.message is None, (cell, ref.message)
        assert len(ref.scalars) == 1 + fc.QUIET_STEPS
        assert not ref.gas[cell]   # (a solid cell: nothing reads its energy)
        for f in fc.fields_of(deck):
            assert np.isfinite(ref.snap[f][ref.gas]).all(), (cell, f)
        # the same march without the poison: the solid cell's energy changed nothing
        c = fc.cpu(deck)
        c.step(fc.POISON_AFTER + 1 + fc.QUIET_STEPS)
        assert not fc.misses_equal(c.field, c.summary(), ref.snap, ref.gas, fc.fields_of(deck))


@pytest.mark.parametrize("deck,geom", [("wedge", g) for g in fc.WEDGE_GEOMS] + [("triple_point", fc.TRIPLE_GEOM)])
def test_geometry_cells_are_what_their_roles_say(hf, native, deck, geom):
    """The cells the GPU tests add for a tile geometry sit where their names
    say; their outcome is the CPU twin's, and they are not all quiet."""
    nx, ny = fc.grid(deck)
    nt, cpt, tj = geom
    T = native.lean_tile_geom(nx, ny, nt, tj, cpt)
    cells = fc.geometry_cells(native, deck, geom)
    assert set(cells) == set(fc.ROLES)
    i, j = cells["tile_first"]
    assert i % T["TI"] == 0 and j % T["TJ"] == 0 and j > 0
    i, j = cells["tile_last"]
    assert (i + 1) % T["TI"] == 0 and (j + 1) % T["TJ"] == 0 and i + 1 < nx and j + 1 < ny
    i, j = cells["partial_tile"]
    assert i // T["TI"] == T["nbi"] - 1 and nx - (T["nbi"] - 1) * T["TI"] < T["TI"] and i < nx
    assert cells["last_row"][1] == ny - 1
    gas = fc.cpu_poison(deck, cells["last_row"]).gas
    assert all(gas[c] for c in cells.values()), cells
    assert len(set(cells.values())) == 4 and not set(cells.values()) & set(fc.POISON[deck].raises)
    outcome = {r: fc.cpu_poison(deck, c).message is not None for r, c in cells.items()}
    print(deck, geom, T, cells, outcome)
    assert any(outcome.values()), outcome


@pytest.mark.parametrize("deck", ["wedge_keps", "step", "resonator", "plate_sst", "sa_adiabatic"])
def test_centre_cell_of_the_viscous_decks_raises(hf, deck):
    """The one poisoned cell of the decks POISON does not list is a gas cell
    and the CPU reports it in the very next step."""
    cell = fc.centre_cell(deck)
    ref = fc.cpu_poison(deck, cell)
    assert ref.gas[cell]
    assert ref.message is not None and "on iteration %d," % fc.POISON_AFTER in ref.message, (cell, ref.message)


@pytest.mark.parametrize("nid", [n.id for n in fc.NATURAL])
def test_natural_failure_iteration(hf, nid):
    """The unpoisoned decks report at the pinned iteration and not before;
    the state the report is made from is kept for the GPU comparison."""
    n = fc.NATURAL_BY_ID[nid]
    ref = fc.cpu_natural(nid)
    assert ref.iteration == n.iteration, ref
    assert "Computational unstability (Tg < 0) on iteration %d," % n.iteration in ref.message, ref.message
    assert len(ref.scalars) == n.iteration and ref.snap is not None
    assert ref.snap["iteration"] == n.iteration
    assert all(dt > 0 and np.isfinite(dt) for dt, _ in ref.scalars)


def test_the_two_spalart_allmaras_rows_differ_only_in_the_wall(hf):
    """isAdiabaticWall 0 and 1 report at the same iteration (the GPU runs the
    first on the split SK_SGT kernels and the second on the lean N-S tiles)."""
    a, b = fc.cpu_natural("sa"), fc.cpu_natural("sa_adiabatic")
    assert a.iteration == b.iteration == 24
    assert "isAdiabaticWall=0" in fc.deck_text("sa") and "isAdiabaticWall=1" in fc.deck_text("sa_adiabatic")


def test_poison_is_seen_differently_by_the_plain_and_the_lean_stepper(hf, tmp_path):
    """The driver's fault injection (and poison_cell) changes rhoE alone: the
    record's stored fluxes stay those of the state before.  The plain stepper
    uses them for one more step, the lean steppers recompute every flux from
    the poisoned state.  So the two CPU steppers, bit for bit the same until
    the poison (the checkpoints) and in the iteration that reports, write
    different error snapshots -- which is why the GPU's lean kernels are
    compared with the lean CPU stepper there (test_gpu_failure_paths.py)."""
    from openhyperflow2d_amd.models import decks

    text = decks.wedge15(80, 30, nmax=20, nout=5)
    text = decks.set_key(decks.set_key(text, "MonitorIndex", 1), "ExitMonitorValue", 1e-30)
    out = {}
    for lean in (False, True):
        d = tmp_path / str(lean)
        d.mkdir()
        sim = hf.Simulation(text, "cpu", workdir=str(d), lean=lean)
        assert sim.solver.lean_ok and sim.solver.lean == lean
        with pytest.raises(RuntimeError, match="on iteration 25,") as ei:
            sim.run(max_cycles=3, outdir=str(d), verbose=True, fault="step:25")
        line = [s for s in str(ei.value).splitlines() if s.startswith("Tg=")]
        assert len(line) == 1
        out[lean] = (line[0], (d / "Wedge15_80x30-err.plt").read_bytes(), (d / "Wedge15_80x30.hf2d").read_bytes())
    assert out[False][2] == out[True][2] and len(out[False][2]) > 0
    assert out[False][1] != out[True][1]
    assert out[False][0] != out[True][0], out[False][0]
