"""Conditions on the CPU reference of tests/model_families.py alone: they keep
the GPU comparison (test_gpu_model_families.py) from passing vacuously -- a
flat field, a y+ or mu_t that never varies, or a NaN would hide a wrong
neighbour, a wrong model constant or a skipped y+ launch."""
import numpy as np
import pytest

from tests import model_families as mf

IDS = [r.id for r in mf.ROWS]


def test_the_table_covers_the_decks():
    """Every fixture deck is either a row or named as left out, and the three
    groups hold what the protocol says."""
    import os

    left_out = {"wall_law", "wedge_keps_wallheat", "step_euler", "oblique_shock", "wedge15_200x40_euler",
                "wedge15_200x60_ns_keps", "restart_from_hf2d"}   # (the last resumes from a checkpoint: no cold start)
    assert {r.deck for r in mf.ROWS} | left_out == set(os.listdir(mf.REF))
    assert len(mf.VISCOUS) == 16 and len(mf.INVISCID) == 12 and len(mf.LNS) == 5
    for r in mf.VISCOUS:
        assert "isAdiabaticWall=0>" in mf.deck_text(r), r.id   # hf2d_wall_solid / hf2d_wall_wall run
        assert "ProblemType=1>" in mf.deck_text(r), r.id
    for r in mf.LNS:
        assert "isAdiabaticWall=1>" in mf.deck_text(r) and "isAdiabaticWall=0>" not in mf.deck_text(r), r.id
    for r in mf.INVISCID:
        assert "ProblemType=0>" in mf.deck_text(r), r.id
        if r.keys:
            assert "<data/BFF=%d>" % r.keys[0][1] in mf.deck_text(r), r.id
    assert [r.id for r in mf.ROWS if r.rule != "equal" and not r.viscous] == ["zeldovich_reacting"]


@pytest.mark.parametrize("rid", IDS)
def test_cpu_reference_is_not_vacuous(rid):
    row = mf.BY_ID[rid]
    ref = mf.cpu_reference(rid)
    gas, first, last = ref.gas, ref.snaps[0], ref.snaps[-1]
    assert ref.flat_start == 0.0
    assert ref.flat_end <= 0.02
    nmax = {"wall_law_plate": 60, "zeldovich_reacting": 20}.get(row.deck, 30)
    assert [s["iteration"] for s in ref.snaps] == [nmax, nmax + 4, nmax + 10, nmax + 13]
    for f in mf.fields_of(row):
        bad = int((~np.isfinite(last[f]) & gas).sum())
        if f in row.nan:
            # the reference's own NaN (module table): there from the first cycle on,
            # on the same cells, and on some cells only
            assert 0 < bad < int(gas.sum()), (f, bad)
            for s in ref.snaps:
                np.testing.assert_array_equal(np.isnan(s[f]), np.isnan(last[f]), err_msg=f)
        else:
            assert bad == 0, (f, bad)
    if not row.viscous:
        return
    assert mf.distinct(first["y_plus"], gas) > 1000
    if row.mu_t == "varied":
        assert mf.distinct(last["mu_t"], gas) >= 1000
    else:
        assert row.mu_t == "const"
        assert mf.distinct(last["mu_t"], gas) <= 3
        mu_t, mu = last["mu_t"][gas], last["mu"][gas]
        assert (mu_t / mu).max() < 6.0
    if row.y_damped:
        # why the cycle is in the protocol: no y+, no damping, one mu_t
        assert mf.distinct(first["mu_t"], gas) == 1
        assert mf.distinct(last["mu_t"], gas) >= 1000
    else:
        assert row.mu_t == "const" or mf.distinct(first["mu_t"], gas) >= 1000


def test_y_damped_rows_are_the_two_the_protocol_names():
    assert sorted({r.deck for r in mf.ROWS if r.y_damped}) == ["keps_chien", "van_driest"]
    assert sorted(r.id for r in mf.ROWS if r.mu_t == "const") == ["integral_model", "spalart_allmaras_start"]
    assert [r.id for r in mf.ROWS if r.nan] == ["spalart_allmaras_start"]


@pytest.mark.parametrize("rid,field", [("keps_rng", "mu_t"), ("van_driest", "y_plus"), ("bff_linear", "p"),
                                       ("spalart_allmaras_start", "S7"), ("integral_model", "mu_t")])
def test_compare_rejects_a_small_error(rid, field):
    """compare() itself: the reference passes against itself, and one gas cell
    off by 1e-8 of the field's max (equal rule: by one ulp; a NaN field: one
    NaN more; a "const" mu_t: one ulp) fails."""
    row = mf.BY_ID[rid]
    ref = mf.cpu_reference(rid)
    snap, gas = ref.snaps[-1], ref.gas
    summ = {"dt": snap["dt"], "time": snap["time"]}
    mf.compare(row, lambda f: snap[f], summ, snap, gas)
    bad = snap[field].copy()
    i, j = np.argwhere(gas & np.isfinite(bad))[-1]
    if field in row.nan:
        bad[i, j] = np.nan
    elif row.rule == "equal" or row.mu_t == "const":
        bad[i, j] = np.nextafter(bad[i, j], np.inf)
    else:
        bad[i, j] += 1e-8 * np.abs(bad[gas]).max()
    with pytest.raises(AssertionError):
        mf.compare(row, lambda f: bad if f == field else snap[f], summ, snap, gas)
    with pytest.raises(AssertionError):
        mf.compare(row, lambda f: snap[f], dict(summ, dt=summ["dt"] * (1 + 1e-8)), snap, gas)
