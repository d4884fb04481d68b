"""The kinetics test cases of tests/kinetics_cases.py on the CPU: every claim
that module makes about its mechanisms and state sets, the host integrator
mech_chem_host against the NumPy oracle point_implicit_step on them (the
figures of kinetics_cases.TABLE), the generated hiprtc mechanism struct
against tools/gen_mech_header.py, the hiprtc compile (host only) and the
sensitivity of the operator to each constant of the structured mechanism.
The device runs of the same cases are in tests/test_gpu_kinetics_edges.py."""
import copy
import os
import sys
import time
import warnings

import numpy as np
import pytest

from openhyperflow2d_amd.ops import chemistry as ch
from openhyperflow2d_amd.ops import mechanism as M
from tests import kinetics_cases as K
from tests.test_chem_rtc import _numbers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# NumPy's vectorised exp / log differ by an ulp between CPU families, so the
# disagreement measured on another machine may exceed the recorded one a little
SLACK = 3.0


def _oracle(m, c):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (the unclamped Newton may overflow where it diverges)
        return M.point_implicit_step(m, c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)


def _converged(m, c, ref, Tref):
    """Cells where the oracle's own (unclamped) Newton solved e(T) = e inside
    the operator's temperature range, judged by its residual."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        Y = (ref / c.rho).T
        res = np.abs(M.mixture_e(m, Y, Tref) - c.e)
        ok = np.isfinite(ref).all(0) & np.isfinite(Tref) & (Tref > 20.0) & (Tref < 6000.0)
        return ok & (res <= 1e-9 * np.abs(M.mixture_cv(m, Y, Tref) * Tref))


def _disagreement(native, m, text, c, cells=None):
    got, Tg = native.mech_chem_host(text, c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)
    ref, Tref = _oracle(m, c)
    s = slice(None) if cells is None else cells(ref, Tref)
    return ch.increment_error(got[:, s], ref[:, s], c.rhoY[:, s]), float(np.abs(Tg - Tref)[s].max()), got, Tg, ref, Tref


@pytest.fixture(scope="module")
def li():
    return M.h2_air_li2004()


@pytest.fixture(scope="module")
def edges(li):
    return K.edge_states(li)


@pytest.fixture(scope="module")
def measured():
    """Figures printed at the end of the module (pytest -s): the table of
    kinetics_cases' docstring."""
    rows = {}
    yield rows
    for k, v in rows.items():
        print("TABLE %-24s %s" % (k, "  ".join("%.2g" % x for x in v)))


def _check_row(measured, key, ie, dT, project=K.PROJECT_BOUND):
    measured[key] = (ie, dT)
    rie, rdT = K.TABLE[key]
    print("%s: increment_error %.3g (recorded %.2g)  |dT| %.3g K (recorded %.2g)" % (key, ie, rie, dT, rdT))
    # (a figure below a tenth of the project bound does not enter the device
    # bound: rounding noise that need not reproduce digit for digit)
    assert ie <= max(SLACK * rie, 0.1 * project[0]) and dT <= max(SLACK * rdT, 0.1 * project[1]), key
    # the bound of the device tests is never below the project's and never
    # more than ten times what two FP64 implementations disagree by
    b = K.bound(key, project)
    assert b[0] >= project[0] and b[1] >= project[1]
    assert b[0] in (project[0], 10 * rie) and b[1] in (project[1], 10 * rdT)


# ---------------------------------------------------------------------------
# the mechanisms
# ---------------------------------------------------------------------------
def test_structured_mechanism_carries_every_reaction_form():
    m = K.structured_mechanism()
    assert m.names == K.STRUCTURED_ORDER and m.ns == 11 and m.names[-1] == "N2"
    rx = m.reactions
    assert 9 <= len(rx) <= 11
    W = {s.name: s.W for s in m.species}
    atoms = {"H2": (2, 0), "O2": (0, 2), "H": (1, 0), "O": (0, 1), "OH": (1, 1), "H2O": (2, 1), "HO2": (1, 2),
             "H2O2": (2, 2)}
    for r in rx:
        for k in (0, 1):   # H and O atoms balance, so mass does
            assert sum(n * atoms[s][k] for s, n in r.reactants.items()) == \
                sum(n * atoms[s][k] for s, n in r.products.items()), r.equation()
        mass = lambda d: sum(n * W[s] for s, n in d.items())
        assert abs(mass(r.reactants) - mass(r.products)) < 1e-5 * mass(r.reactants)
        assert not set(K.INERTS) & (set(r.reactants) | set(r.products))
    assert any(3 in r.reactants.values() and r.b == 0 and r.Ta == 0 for r in rx)
    assert any(not r.reversible and r.b == 0 and r.Ta == 0 for r in rx)
    assert any(r.third_body and not r.falloff and not r.eff for r in rx)
    assert any(r.third_body and {"AR", "HE"} <= set(r.eff) for r in rx)
    assert any(r.falloff and not r.troe for r in rx)
    assert any(r.falloff and r.troe and len(r.troe) == 4 and all(1.0 < t < 1e5 for t in r.troe[1:]) for r in rx)
    assert any(len(r.reactants) == 3 and len(r.products) == 3 for r in rx)
    assert {sum(r.products.values()) - sum(r.reactants.values()) for r in rx} == {-1, 0, 1}
    assert sum(1 for r in rx if r.equation() in {q.equation() for q in M.h2_air_li2004().reactions}) >= 3
    for clone in ("AR", "HE"):
        assert m.species[m.index(clone)].low == m.species[-1].low
    assert m.slots["air"]["AR"] > 0 and m.slots["fuel"] == {"H2": 1.0}
    # the file form round-trips
    assert M.Mechanism.from_text(m.to_text()).to_text() == m.to_text()


def test_permuted_and_frozen_mechanisms():
    m = K.structured_mechanism()
    p = K.permuted(m)
    assert sorted(p.names) == sorted(m.names) and p.names != m.names
    assert p.names[-3:] == ["N2", "HE", "AR"]     # inerts last, none of them where it was
    assert [r.equation() for r in p.reactions] == [r.equation() for r in m.reactions]
    ix = K.permutation(m, p)
    assert [m.names[i] for i in ix] == p.names
    f = K.frozen_mechanism()
    assert f.names == m.names and f.nr == 0
    # the same physical states for both orders
    a, b = K.structured_states(m)[0], K.structured_states(p)[0]
    np.testing.assert_array_equal(a.rhoY[ix], b.rhoY)
    np.testing.assert_array_equal(a.rho, b.rho)
    np.testing.assert_allclose(a.e, b.e, rtol=1e-12)


# ---------------------------------------------------------------------------
# the state sets
# ---------------------------------------------------------------------------
def test_edge_state_sets_are_what_they_say(li, edges):
    names = {"cold", "tmid", "far_guess", "clamped_guess", "no_radicals", "no_fuel", "bath_only", "negative", "thin",
             "dense", "stiff", "sizes"}
    assert set(edges) == names
    ix = li.index
    for name, cases in edges.items():
        for c in cases:
            assert c.rhoY.shape == (li.ns, c.rho.size) and c.e.shape == c.T0.shape == c.rho.shape
            assert c.rho.size <= 400
            # the radical levels of test_gpu_mechanism._states, not raised
            for s, lvl in K.H2AIR_SCALE.items():
                assert (c.rhoY[ix(s)] / c.rho).max() <= lvl, (name, s)
    c = edges["cold"][0]
    assert c.rho.size == 400 and c.T0[0] == 100.0 and c.T0[-1] == 400.0 and (np.diff(c.T0) > 0).all()
    T = edges["tmid"][0].T0
    assert T.min() == 999.9 and T.max() == 1000.1
    for v in (1000.0, np.nextafter(1000.0, 0.0), np.nextafter(1000.0, 2000.0)):
        assert (T == v).any()
    (a, b), (lo, hi) = edges["far_guess"], edges["clamped_guess"]
    assert (a.T0 == 300.0).all() and (b.T0 == 5500.0).all() and (lo.T0 == 5.0).all() and (hi.T0 == 1e4).all()
    for c in (b, lo, hi):
        np.testing.assert_array_equal(c.rhoY, a.rhoY)
        np.testing.assert_array_equal(c.e, a.e)
    Tsol = M.T_from_e(li, (a.rhoY / a.rho).T, a.e, T0=1500.0)
    assert Tsol.min() > 899 and Tsol.max() < 2701
    c = edges["no_radicals"][0]
    for s in ("H", "O", "OH", "HO2", "H2O2"):
        assert (c.rhoY[ix(s)] == 0.0).all()
    assert (c.rhoY[ix("H2")] > 0).all()
    c = edges["no_fuel"][0]
    assert (c.rhoY[ix("H2")] == 0.0).all() and (c.rhoY[ix("O2")] == 0.0).all() and (c.rhoY[ix("OH")] > 0).all()
    c = edges["bath_only"][0]
    assert (c.rhoY[:-1] == 0.0).all() and (c.rhoY[-1] == c.rho).all() and (c.dt, c.nsub) == (1e-6, 2)
    c = edges["negative"][0]
    assert ((c.rhoY < 0).sum(0) == 1).all() and c.rhoY.min() == -1e-12
    assert len({int(k) for k in np.argmin(c.rhoY, 0)}) == 5
    c = edges["thin"][0]
    assert 1e-4 <= c.rho.min() and c.rho.max() <= 2e-4
    c = edges["dense"][0]
    assert 20 <= c.rho.min() and c.rho.max() <= 50
    assert [(c.dt, c.nsub) for c in edges["stiff"]] == [(1e-3, 1), (1e-2, 1)]
    assert [c.rho.size for c in edges["sizes"]] == [1, 15, 16, 17, 63, 64, 65, 255, 256, 257]
    full = edges["sizes"][-1]
    for c in edges["sizes"]:
        k = c.rho.size
        np.testing.assert_array_equal(c.rhoY, full.rhoY[:, :k])
        np.testing.assert_array_equal(c.e, full.e[:k])
    for name in names - {"bath_only", "stiff"}:
        assert all((c.dt, c.nsub) == (1e-7, 2) for c in edges[name]), name


def test_cold_set_stays_inside_the_oracle_domain(li):
    """Below about 72 K the oracle's reverse rate of H2 + M <=> 2 H + M
    overflows (the exponent of its equilibrium constant): the cold set starts
    at 100 K, where every rate is finite."""
    c = np.full((2, li.ns), 1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        kf, kr, _, _ = M.rate_parts(li, c, np.array([60.0, 100.0]))
    j = [r.equation() for r in li.reactions].index("H2 + M <=> 2 H + M")
    assert not np.isfinite(kr[0, j]) and np.isfinite(kr[1]).all() and np.isfinite(kf).all()


@pytest.mark.parametrize("name", ["cold", "tmid", "no_radicals", "no_fuel", "bath_only", "negative", "thin", "dense",
                                  "stiff", "sizes"])
def test_host_matches_oracle_on_edge_states(native, li, edges, measured, name):
    """mech_chem_host against point_implicit_step on every set whose guess is
    near its solution, and on the cold set where NumPy's Newton converges."""
    worst = [0.0, 0.0]
    for c in edges[name]:
        cells = (lambda ref, Tref: _converged(li, c, ref, Tref)) if name == "cold" else None
        ie, dT, got, Tg, ref, Tref = _disagreement(native, li, "h2_air_li2004", c, cells)
        worst = [max(worst[0], ie), max(worst[1], dT)]
        assert np.isfinite(got).all() and np.isfinite(Tg).all()
        if name == "cold":
            ok = _converged(li, c, ref, Tref)
            print("cold: NumPy's Newton converges in %d of %d cells" % (ok.sum(), ok.size))
            assert ok.sum() >= ok.size // 2
        else:
            assert np.isfinite(ref).all() and np.isfinite(Tref).all()
        assert (got >= 0).all() and (ref[:, np.isfinite(ref).all(0)] >= 0).all()
        # mass: sum rhoY = rho
        assert np.abs(got.sum(0) - c.rho).max() <= 1e-15 * c.rho.max()
        if name == "bath_only":
            for out, T in ((got, Tg), (ref, Tref)):
                assert K.unchanged(out, c) and (out[:-1] == 0.0).all()
                assert np.abs(T - c.T0).max() <= 1e-12 * c.T0.max()
        if name in ("stiff", "dense"):
            print("%s dt=%g: T up to %.0f K" % (name, c.dt, Tg.max()))
            assert Tg.max() > 4000.0     # the step limit and a long way from the guess
    _check_row(measured, "h2air:" + name, *worst)


def test_host_solution_does_not_depend_on_the_guess(native, li, edges):
    """far_guess / clamped_guess: the clamped, step-limited Newton of the host
    integrator reaches the solution of the near guess from 300, 5500, 5 and
    1e4 K; these sets are compared with mech_chem_host, not with NumPy's
    unclamped Newton."""
    a = edges["far_guess"][0]
    Tnear = M.T_from_e(li, (a.rhoY / a.rho).T, a.e, T0=1500.0)
    ref, Tref = native.mech_chem_host("h2_air_li2004", a.rhoY, a.rho, a.e, Tnear, a.dt, a.nsub)
    for c in edges["far_guess"] + edges["clamped_guess"]:
        got, Tg = native.mech_chem_host("h2_air_li2004", c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)
        assert np.isfinite(got).all()
        assert ch.increment_error(got, ref, c.rhoY) < 1e-9 and np.abs(Tg - Tref).max() < 1e-8, c.T0[0]


def test_host_prefixes_reproduce_the_full_result(native, edges):
    full = edges["sizes"][-1]
    ref, Tref = native.mech_chem_host("h2_air_li2004", full.rhoY, full.rho, full.e, full.T0, full.dt, full.nsub)
    for c in edges["sizes"]:
        got, Tg = native.mech_chem_host("h2_air_li2004", c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)
        np.testing.assert_array_equal(got, ref[:, :c.rho.size])
        np.testing.assert_array_equal(Tg, Tref[:c.rho.size])


@pytest.mark.parametrize("which", ["structured", "permuted"])
def test_host_matches_oracle_on_structured_mechanism(native, measured, which):
    m = K.structured_mechanism()
    if which == "permuted":
        m = K.permuted(m)
    inert = [m.index(s) for s in K.INERTS]
    text = m.to_text()
    sets = {"unclipped": K.structured_states(m, K.UNCLIPPED), "clipped": K.structured_states(m, [K.CLIPPED]),
            "cool": K.cool_states(m)}
    for label, cases in sets.items():
        worst = [0.0, 0.0]
        for c in cases:
            ie, dT, got, Tg, ref, Tref = _disagreement(native, m, text, c)
            worst = [max(worst[0], ie), max(worst[1], dT)]
            assert np.isfinite(ref).all() and np.isfinite(got).all()
            assert np.abs(got.sum(0) - c.rho).max() <= 1e-15 * c.rho.max()
            moved = np.abs(ref[inert] / c.rhoY[inert] - 1.0).max()
            if label == "clipped":
                # the clip removes mass and the re-normalisation moves the inerts:
                # part of the operator, compared with the host integrator only
                assert moved > 1e-3 and np.abs(got[inert] / c.rhoY[inert] - 1.0).max() > 1e-3
            else:
                assert moved <= 1e-12
        _check_row(measured, which + ":" + label, *worst)


def test_permuted_host_result_is_the_original_permuted(native):
    """Not bit for bit: the two eliminate in different orders."""
    m = K.structured_mechanism()
    p = K.permuted(m)
    ix = K.permutation(m, p)
    for a, b in zip(K.structured_states(m) + K.cool_states(m), K.structured_states(p) + K.cool_states(p)):
        ya, Ta = native.mech_chem_host(m.to_text(), a.rhoY, a.rho, a.e, a.T0, a.dt, a.nsub)
        yb, Tb = native.mech_chem_host(p.to_text(), b.rhoY, b.rho, b.e, b.T0, b.dt, b.nsub)
        assert ch.increment_error(yb, ya[ix], b.rhoY) < K.PROJECT_BOUND[0]
        assert np.abs(Ta - Tb).max() < K.PROJECT_BOUND[1]


def test_frozen_mechanism_returns_its_input(native, measured):
    m = K.frozen_mechanism()
    c, = K.frozen_states(m)
    assert (c.dt, c.nsub) == (1e-6, 2)
    ie, dT, got, Tg, ref, Tref = _disagreement(native, m, m.to_text(), c)
    for out, To in ((got, Tg), (ref, Tref)):
        assert K.unchanged(out, c)
        assert np.abs(To - c.T0).max() <= 1e-12 * c.T0.max()
    _check_row(measured, "frozen", ie, dT)


@pytest.mark.parametrize("ns,nr", K.RANDOM_SIZES)
def test_host_matches_oracle_on_random_mechanisms(native, measured, ns, nr):
    m, Y, rho, e, T = K.random_case(ns, nr)
    worst = [0.0, 0.0]
    for dt, nsub in K.UNCLIPPED + [K.CLIPPED]:
        ie, dT, got, Tg, ref, Tref = _disagreement(native, m, m.to_text(), K.Case(Y, rho, e, T, dt, nsub))
        assert np.isfinite(ref).all()
        worst = [max(worst[0], ie), max(worst[1], dT)]
    _check_row(measured, "random:%d,%d" % (ns, nr), *worst, project=K.RANDOM_BOUND)


# ---------------------------------------------------------------------------
# the generated mechanism struct and its hiprtc compile
# ---------------------------------------------------------------------------
def _mechanisms():
    s = K.structured_mechanism()
    return [s, K.permuted(s), K.frozen_mechanism()] + [K.random_mech(ns, nr, ns) for ns, nr in K.RANDOM_SIZES]


@pytest.mark.parametrize("k", range(7))
def test_generated_struct_matches_the_header_generator(native, k):
    """C++ mech_struct_source == tools/gen_mech_header.py, number for number,
    beyond the built-in mechanism: species permutations, an empty reaction
    table, every reaction form."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gen_mech_header import header

    m = _mechanisms()[k]
    want = _numbers(header(m))
    got = _numbers(native.mech_struct_source(m.to_text()))
    assert len(want) > 14 * m.ns + 19 * m.nr and got == want, m.name


@pytest.mark.parametrize("k", range(7))
def test_hiprtc_compiles_or_refuses_with_a_reason(native, tmp_path, monkeypatch, k):
    monkeypatch.setenv("HF2D_RTC_CACHE", str(tmp_path / "cache"))
    m = _mechanisms()[k]
    t = time.perf_counter()
    n, cached, why = native.chem_rtc_compile(m.to_text())
    t = time.perf_counter() - t
    print("hiprtc %s (%d species, %d reactions): %d bytes, %.1f s" % (m.name, m.ns, m.nr, n, t))
    if m.nr == 0:
        # a zero-length reaction table is not C++: refused before the compiler sees it
        assert n < 0 and "without reactions" in why
    else:
        assert n > 10000 and not cached, why
        assert t < 60.0    # (beyond a few tens of seconds the device tests would use a smaller mechanism)
    assert n > 0 or why.strip()


# ---------------------------------------------------------------------------
# sensitivity: a wrong number in the generated struct cannot hide under the bound
# ---------------------------------------------------------------------------
def _perturbed(feature, f=1.0 + 1e-6):
    m = copy.deepcopy(K.structured_mechanism())
    rx = {r.equation(): r for r in m.reactions}
    if feature == "lindemann A0":
        rx["H + O2 (+M) <=> HO2 (+M)"].A0 *= f
    elif feature.startswith("troe"):
        r = rx["H2O2 (+M) <=> 2 OH (+M)"]
        t = list(r.troe)
        t[int(feature[-1])] *= f
        r.troe = tuple(t)
    elif feature == "eff AR":
        rx["H2 + M <=> 2 H + M"].eff["AR"] *= f
    elif feature == "A coefficient 3":
        rx["3 H <=> H2 + H"].A *= f
    elif feature == "A three species":
        rx["H2O2 + H + O <=> H2 + O2 + OH"].A *= f
    elif feature == "A irreversible":
        rx["HO2 + O => O2 + OH"].A *= f
    else:
        raise KeyError(feature)
    return m


@pytest.mark.parametrize("feature,states", [
    ("lindemann A0", "unclipped"), ("troe 1", "cool"), ("troe 2", "unclipped"), ("troe 3", "unclipped"),
    ("eff AR", "cool"), ("A coefficient 3", "cool"), ("A three species", "unclipped"),
    ("A irreversible", "unclipped")])
def test_one_constant_changed_by_1e_6_exceeds_the_device_bound(native, feature, states):
    """mech_chem_host with one constant of the structured mechanism changed by
    1e-6 relative differs from the unperturbed one by more than the bound the
    device kernels are held to on the same state set (the warm set, or the
    cool one for the terms that are invisible above 900 K)."""
    m = K.structured_mechanism()
    p = _perturbed(feature)
    assert p.to_text() != m.to_text()
    cases = K.cool_states(m) if states == "cool" else K.structured_states(m, K.UNCLIPPED)
    limit = K.bound("structured:" + states)[0]
    for c in cases:
        base, _ = native.mech_chem_host(m.to_text(), c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)
        got, _ = native.mech_chem_host(p.to_text(), c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)
        ie = ch.increment_error(got, base, c.rhoY)
        print("%s, %s dt=%g/%d: increment_error %.3g (bound %.2g)" % (feature, states, c.dt, c.nsub, ie, limit))
        assert ie > limit
