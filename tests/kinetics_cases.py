"""Mechanisms and state sets for the kinetics kernels' tests (plain module, no
fixtures; tests/test_kinetics_cases.py checks every claim made here on the
CPU, tests/test_gpu_kinetics_edges.py runs the sets through the device
kernels).

Mechanisms
  structured_mechanism()  11 species (the H2/air set + two inert N2 clones, AR
                          listed first and HE in the middle, N2 last) and ten
                          mass-conserving steps that together carry every field
                          of a CRx record: coefficient 3, constant-rate steps
                          (b = Ta = 0) reversible and irreversible, "+ M" with
                          and without an efficiency row, Lindemann and
                          4-parameter Troe fall-off, three species per side,
                          dnu = -1, 0, +1.
  permuted(m, order)      the same mechanism with its species reordered.
  frozen_mechanism()      the same species, no reactions.
  random_mech / random_case  the random mechanisms of tests/test_chem_mech.py.

State sets: edge_states(m) for the H2/air set; structured_states(m) (warm,
at two (dt, nsub) pairs that clip nothing and one that does) and
cool_states(m) for the structured one; frozen_states(m).  Every entry is a
Case(rhoY, rho, e, T0, dt, nsub).

Measured on the CPU (tests/test_kinetics_cases.py re-measures and asserts
them): the disagreement of the two independent FP64 implementations
mech_chem_host (C++) and point_implicit_step (NumPy) per set, the hiprtc
compile wall time of each mechanism, and the device-against-host bound that
follows (TABLE below: the project bound, or ten times the CPU disagreement
where that exceeds a tenth of the project bound -- the conditioning floor).

  set                    CPU disagreement        device bound
                         incr.err   |dT| K       incr.err   |dT| K
  h2air:cold             2.1e-12    2.8e-12      1e-09      1e-08
  h2air:tmid             4.6e-10    1.9e-10      4.6e-09    1e-08
  h2air:no_radicals      2.3e-10    1.4e-12      2.3e-09    1e-08
  h2air:no_fuel          2.1e-10    9.1e-13      2.1e-09    1e-08
  h2air:bath_only        0          1.4e-12      1e-09      1e-08
  h2air:negative         9.3e-14    1.4e-12      1e-09      1e-08
  h2air:thin             1.5e-10    1.4e-12      1.5e-09    1e-08
  h2air:dense            2.7e-13    1.3e-10      1e-09      1e-08
  h2air:stiff            1.4e-11    4.1e-09      1e-09      4.1e-08
  h2air:sizes            1.4e-10    1.4e-12      1.4e-09    1e-08
  h2air:far_guess, clamped_guess  (host only)    1e-09      1e-08
  structured:unclipped   2.9e-10    1.4e-12      2.9e-09    1e-08
  structured:clipped     4.6e-14    6.4e-12      1e-09      1e-08
  structured:cool        2.2e-10    8.0e-13      2.2e-09    1e-08
  permuted:unclipped     2.9e-10    1.4e-12      2.9e-09    1e-08
  permuted:clipped       1.1e-13    3.0e-12      1e-09      1e-08
  permuted:cool          2.2e-10    9.1e-13      2.2e-09    1e-08
  frozen                 1.7e-10    1.4e-12      1.7e-09    1e-08
  random:3,5             9.6e-14    9.1e-13      1e-07      1e-06
  random:10,17           4.2e-10    1.4e-12      1e-07      1e-06
  random:13,21           4.7e-09    2.6e-11      1e-07      1e-06
  random:16,40           1.4e-12    1.4e-12      1e-07      1e-06

(The 1e-10 .. 5e-10 increment errors are one ulp of the inert bath gas against
increment_error's floor of 1e-6 of the species' level; the reacting species
agree to 1e-12 and better.  The stiff steps end up to 3100 K from their guess,
the dense ones up to 3800 K; the clipped pair moves the inerts by 4 %.)

hiprtc compile, one core, cold cache: structured 1.8 s, permuted 2.2 s,
rand3 0.6 s, rand10 2.4 s, rand13 5.7 s, rand16 (16 species, 38 steps) 7.1 s,
so the device tests run hiprtc on every one of them; frozen (no reactions) is
refused with a reason before the compiler is called.

Sensitivity (mech_chem_host with one constant changed by 1e-6 relative
against the unperturbed one, smallest increment error over the set's pairs):
  warm set (bound 2.9e-09): Lindemann A0 8.0e-07, troe[2] 1.9e-07, troe[3]
    3.1e-07, A of the three-species step 7.8e-09, A of the irreversible
    constant-rate step 6.8e-08
  cool set (bound 2.2e-09): troe[1] 6.2e-08, AR efficiency 1.4e-08, A of the
    coefficient-3 step 3.7e-08
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from openhyperflow2d_amd.ops import mechanism as M

Case = namedtuple("Case", "rhoY rho e T0 dt nsub")

STRUCTURED_ORDER = ["AR", "H2", "O2", "H", "HE", "O", "OH", "H2O", "HO2", "H2O2", "N2"]
PERMUTED_ORDER = ["H2O2", "OH", "H2", "O", "HO2", "H2O", "O2", "H", "N2", "HE", "AR"]   # inerts last
INERTS = ("AR", "HE", "N2")

# test_gpu_mechanism._states' species levels (H2/air order), by name
H2AIR_SCALE = {"H2": 0.03, "O2": 0.2, "H2O": 0.1, "H": 1e-3, "O": 1e-3, "OH": 3e-3, "HO2": 1e-4, "H2O2": 1e-5}
STRUCTURED_SCALE = {"AR": 0.05, "H2": 0.03, "O2": 0.2, "H": 1e-4, "HE": 0.05, "O": 1e-3, "OH": 3e-3, "H2O": 0.1,
                    "HO2": 1e-4, "H2O2": 1e-5}

UNCLIPPED = [(1e-8, 1), (1e-7, 2)]
CLIPPED = (1e-6, 4)

# project bounds of the device kernels against the host integrator
# (increment_error, |dT| in K): tests/test_gpu_mechanism.py, tests/test_chem_mech.py
PROJECT_BOUND = (1e-9, 1e-8)
RANDOM_BOUND = (1e-7, 1e-6)


# ---------------------------------------------------------------------------
# mechanisms
# ---------------------------------------------------------------------------
def _rx(eq, A, b=0.0, Ta=0.0, **kw):
    """A Reaction from an equation in the file syntax and SI constants."""
    text = "%s A=%.17g b=%.17g Ta=%.17g" % (eq, A, b, Ta)
    r = M._parse_reaction(text.split())
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def structured_reactions():
    li = {r.equation(): r for r in M.Mechanism.load(M.DATA_DIR + "/h2_air_li2004.mech").reactions}
    fo = li["H + O2 (+M) <=> HO2 (+M)"]
    dec = li["H2O2 (+M) <=> 2 OH (+M)"]
    diss = li["H2 + M <=> 2 H + M"]
    return [
        # three ordinary Li et al. steps with their SI constants
        li["H + O2 <=> O + OH"],
        li["O + H2 <=> H + OH"],
        li["H2 + OH <=> H2O + H"],
        # coefficient 3, constant rate, dnu = -1
        _rx("3 H <=> H2 + H", 3.2e3),
        # irreversible, constant rate
        _rx("HO2 + O => O2 + OH", 3.25e7),
        # "+ M" without efficiencies (eff == -1), dnu = -1
        _rx("O + H <=> OH", 4.714e6, -1.0, 0.0, third_body=True),
        # "+ M" whose efficiencies name the two added inerts, dnu = +1
        _rx("H2 <=> 2 H", diss.A, diss.b, diss.Ta, third_body=True,
            eff={"AR": 0.75, "HE": 0.65, "H2": 2.5, "H2O": 12.0}),
        # Lindemann fall-off (no troe)
        _rx("H + O2 <=> HO2", fo.A, fo.b, fo.Ta, falloff=True, A0=fo.A0, b0=fo.b0, Ta0=fo.Ta0,
            eff={"H2": 2.0, "H2O": 11.0, "O2": 0.78}),
        # 4-parameter Troe with finite T3, T1, T2
        _rx("H2O2 <=> 2 OH", dec.A, dec.b, dec.Ta, falloff=True, A0=dec.A0, b0=dec.b0, Ta0=dec.Ta0,
            troe=(0.5, 90.0, 1200.0, 4500.0), eff={"H2": 2.5, "H2O": 12.0}),
        # three distinct species on each side (H3 O3 = H3 O3), dnu = 0
        _rx("H2O2 + H + O <=> H2 + O2 + OH", 2.0e7, 0.5, 1000.0),
    ]


def _species(order):
    base = {s.name: s for s in M.h2_air_li2004().species}
    n2 = base["N2"]
    for clone in ("AR", "HE"):
        base[clone] = M.Species(clone, n2.W, n2.Tlo, n2.Tmid, n2.Thi, n2.low, n2.high, n2.sigma, n2.eps_k)
    return [base[s] for s in order]


def _slots():
    slots = dict(M.Mechanism.load(M.DATA_DIR + "/h2_air_li2004.mech").slots)
    # the first-listed inert has a non-zero concentration in a deck
    slots["air"] = {"N2": 0.9, "AR": 0.1}
    return slots


def structured_mechanism():
    return M.Mechanism("structured", _species(STRUCTURED_ORDER), structured_reactions(), _slots())


def frozen_mechanism():
    return M.Mechanism("frozen", _species(STRUCTURED_ORDER), [], _slots())


def permuted(m, order=PERMUTED_ORDER):
    """The mechanism m with its species listed in `order`."""
    by = {s.name: s for s in m.species}
    assert sorted(order) == sorted(by)
    return M.Mechanism(m.name + "_perm", [by[s] for s in order], list(m.reactions), dict(m.slots))


def permutation(m, mp):
    """Row index into a state of m for every species of mp: y_p = y[ix]."""
    return np.array([m.index(s) for s in mp.names])


def random_mech(ns, nr, seed, reversible=True):
    """Random mechanism over species of equal molar mass (so a step conserves
    mass when its coefficient sums agree), reversible / irreversible / third-body
    steps of orders 1..3."""
    rng = np.random.default_rng(seed)
    n2 = M.h2_air_li2004().species[-1]
    sp = []
    for i in range(ns):
        # N2-like thermo with the formation enthalpy / entropy constants shifted by
        # up to +-2000 K / +-2: moderate equilibrium constants and heat release
        lo, hi = list(n2.low), list(n2.high)
        dh, ds = rng.uniform(-2000, 2000), rng.uniform(-2, 2)
        lo[5] += dh
        hi[5] += dh
        lo[6] += ds
        hi[6] += ds
        sp.append(M.Species("S%d" % i, 0.02, n2.Tlo, n2.Tmid, n2.Thi, lo, hi, n2.sigma, n2.eps_k))
    names = [s.name for s in sp]
    rx = []
    for r in range(nr):
        k = int(rng.integers(1, 4))
        reac = {names[i]: int(rng.integers(1, 3)) for i in rng.choice(ns, size=k, replace=False)}
        order = sum(reac.values())
        # equal molar masses: mass balance <=> equal total coefficients
        pk = int(rng.integers(1, min(3, order) + 1))
        prods = list(rng.choice(ns, size=pk, replace=False))
        prod = {names[i]: 0 for i in prods}
        for t in range(order):
            prod[names[prods[t % pk]]] += 1
        if any(v > 3 for v in prod.values()):
            prod = {names[prods[0]]: min(order, 3)}
            if order > 3:
                continue
            prod[names[prods[0]]] = order
        tb = bool(rng.random() < 0.2)
        rx.append(M.Reaction(reac, prod, float(10 ** rng.uniform(-1, 2)), float(rng.uniform(-1, 1)),
                             float(rng.uniform(0, 3000)), reversible=reversible and bool(rng.random() < 0.7),
                             third_body=tb, eff={names[0]: 2.0} if tb else {}))
    return M.Mechanism("rand%d" % seed, sp, rx)


def random_case(ns, nr):
    m = random_mech(ns, nr, ns)
    rng = np.random.default_rng(ns + nr)
    n = 16 * 9 + 7
    Y = rng.random((ns, n)) * 0.05 + 1e-4
    T = 900.0 + 1500.0 * rng.random(n)
    rho = Y.sum(0)
    return m, Y, rho, M.mixture_e(m, (Y / rho).T, T), T


RANDOM_SIZES = [(3, 5), (10, 17), (13, 21), (16, 40)]


# ---------------------------------------------------------------------------
# states
# ---------------------------------------------------------------------------
N_CELLS = 16 * 12 + 11   # 203: partial last MFMA tile, partial last wavefront


def _fractions(m, n, rng, scale):
    """Mass fractions [ns, n]: species s uniform in [0, scale[s]), the last
    species of the mechanism's bath gas N2 takes the rest."""
    Y = np.zeros((m.ns, n))
    # one draw per species in a fixed (sorted) name order: a permuted mechanism
    # gets the same physical state
    tot = np.zeros(n)
    for s in sorted(scale):
        Y[m.index(s)] = rng.random(n) * scale[s]
        tot += Y[m.index(s)]
    Y[m.index("N2")] = 1.0 - tot
    return Y


def _state(m, Y, T, rho):
    return rho * Y, rho, M.mixture_e(m, Y.T, T)


def warm(m, n=N_CELLS, seed=3, scale=None):
    """test_gpu_mechanism._states' kind of state: (rhoY, rho, e, T)."""
    rng = np.random.default_rng(seed)
    Y = _fractions(m, n, rng, scale or H2AIR_SCALE)
    T = 900 + 1800 * rng.random(n)
    rho = 0.05 + 0.5 * rng.random(n)
    return (*_state(m, Y, T, rho), T)


SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257]


def edge_states(m):
    """State sets for the H2/air mechanism m: {name: [Case, ...]}."""
    out = {}
    n = N_CELLS
    rng = np.random.default_rng(17)

    def case(Y, T, rho, dt=1e-7, nsub=2, T0=None):
        rhoY, rho, e = _state(m, Y, T, rho)
        return Case(rhoY, rho, e, np.array(T if T0 is None else np.broadcast_to(float(T0), T.shape)), dt, nsub)

    def rho_of(k):
        return 0.05 + 0.5 * rng.random(k)

    def T_of(k):
        return 900 + 1800 * rng.random(k)

    Y = _fractions(m, 400, rng, H2AIR_SCALE)
    out["cold"] = [case(Y, np.linspace(100.0, 400.0, 400), rho_of(400))]

    T = np.concatenate([np.linspace(999.9, 1000.1, 61),
                        [1000.0, np.nextafter(1000.0, 0.0), np.nextafter(1000.0, 2000.0)]])
    out["tmid"] = [case(_fractions(m, T.size, rng, H2AIR_SCALE), T, rho_of(T.size))]

    Y, T, rho = _fractions(m, n, rng, H2AIR_SCALE), T_of(n), rho_of(n)
    out["far_guess"] = [case(Y, T, rho, T0=300.0), case(Y, T, rho, T0=5500.0)]
    out["clamped_guess"] = [case(Y, T, rho, T0=5.0), case(Y, T, rho, T0=1e4)]

    Y = _fractions(m, n, rng, H2AIR_SCALE)
    for s in ("H", "O", "OH", "HO2", "H2O2"):
        Y[m.index(s)] = 0.0
    Y[m.index("N2")] = 0.0
    Y[m.index("N2")] = 1.0 - Y.sum(0)
    out["no_radicals"] = [case(Y, T_of(n), rho_of(n))]

    Y = _fractions(m, n, rng, H2AIR_SCALE)
    for s in ("H2", "O2"):
        Y[m.index(s)] = 0.0
    Y[m.index("N2")] = 0.0
    Y[m.index("N2")] = 1.0 - Y.sum(0)
    out["no_fuel"] = [case(Y, T_of(n), rho_of(n))]

    Y = np.zeros((m.ns, n))
    Y[m.index("N2")] = 1.0
    out["bath_only"] = [case(Y, T_of(n), rho_of(n), dt=1e-6)]

    # one minor species slightly negative (a different one from cell to cell;
    # the major ones carry the energy e was computed with)
    c = case(_fractions(m, n, rng, H2AIR_SCALE), T_of(n), rho_of(n))
    rhoY = c.rhoY.copy()
    minor = np.array([m.index(s) for s in ("H", "O", "OH", "HO2", "H2O2")])
    rhoY[minor[np.arange(n) % minor.size], np.arange(n)] = -1e-12
    out["negative"] = [c._replace(rhoY=rhoY)]

    out["thin"] = [case(_fractions(m, n, rng, H2AIR_SCALE), T_of(n), 1e-4 + 1e-4 * rng.random(n))]
    out["dense"] = [case(_fractions(m, n, rng, H2AIR_SCALE), T_of(n), 20.0 + 30.0 * rng.random(n))]

    Y, T, rho = _fractions(m, n, rng, H2AIR_SCALE), T_of(n), rho_of(n)
    out["stiff"] = [case(Y, T, rho, dt=1e-3, nsub=1), case(Y, T, rho, dt=1e-2, nsub=1)]

    full = case(_fractions(m, 257, rng, H2AIR_SCALE), T_of(257), rho_of(257))
    out["sizes"] = [Case(full.rhoY[:, :k].copy(), full.rho[:k].copy(), full.e[:k].copy(), full.T0[:k].copy(), full.dt,
                         full.nsub) for k in SIZES]
    return out


# sets whose guess is near the solution: the NumPy oracle (unclamped Newton) applies
NEAR_GUESS = ("tmid", "no_radicals", "no_fuel", "bath_only", "negative", "thin", "dense", "stiff", "sizes")


def structured_states(m, pairs=None):
    """Warm states of the structured mechanism (or a permutation of it: the
    same physical states) at the two unclipped (dt, nsub) pairs and the
    clipped one."""
    rhoY, rho, e, T = warm(m, seed=5, scale=STRUCTURED_SCALE)
    return [Case(rhoY, rho, e, T, dt, nsub) for dt, nsub in (pairs or UNCLIPPED + [CLIPPED])]


# In the warm states the Troe T3 = 90 K term (exp(-T / 90)), the AR share of
# the collider of H2 + M <=> 2 H + M and 3 H <=> H2 + H are below 1e-3 of every
# species' increment.  They carry it in a cool mixture without O2 (no
# H + O2 (+M) sink of H, OH + OH (+M) -> H2O2 recombining) at a higher H level.
COOL_SCALE = dict(STRUCTURED_SCALE, O2=0.0, H=2e-3, H2O2=1e-3)


def cool_states(m):
    """The structured mechanism's second state set: 250-600 K, no O2."""
    rng = np.random.default_rng(23)
    n = N_CELLS
    Y = _fractions(m, n, rng, COOL_SCALE)
    T = 250 + 350 * rng.random(n)
    rho = 0.05 + 0.5 * rng.random(n)
    rhoY, rho, e = _state(m, Y, T, rho)
    return [Case(rhoY, rho, e, T, dt, nsub) for dt, nsub in UNCLIPPED]


def frozen_states(m):
    rhoY, rho, e, T = warm(m, seed=5, scale=STRUCTURED_SCALE)
    return [Case(rhoY, rho, e, T, 1e-6, 2)]


def unchanged(got, c):
    """Output equals input to 2 ulp of the cell's density: the operator goes
    through c = rhoY / W, the re-normalisation rho / sum(c W) and rhoY = c W, each
    a rounding at the level of rho (the host integrator and the NumPy oracle
    reach 3 ulp of a single entry and 2 ulp of rho)."""
    return bool((np.abs(got - c.rhoY) <= 2 * np.spacing(c.rho)).all())


def bound(key, project=PROJECT_BOUND):
    """(increment_error, |dT|) bound of a device kernel against mech_chem_host
    for the set `key` of TABLE."""
    ie, dT = TABLE[key][:2]
    return (max(project[0], 10 * ie) if ie > 0.1 * project[0] else project[0],
            max(project[1], 10 * dT) if dT > 0.1 * project[1] else project[1])


# key: (increment_error, |dT| K) of mech_chem_host against point_implicit_step,
# rounded up to two digits as measured by tests/test_kinetics_cases.py
TABLE = {
    "h2air:cold": (2.1e-12, 2.8e-12),
    "h2air:tmid": (4.6e-10, 1.9e-10),
    "h2air:no_radicals": (2.3e-10, 1.4e-12),
    "h2air:no_fuel": (2.1e-10, 9.1e-13),
    "h2air:bath_only": (0.0, 1.4e-12),
    "h2air:negative": (9.3e-14, 1.4e-12),
    "h2air:thin": (1.5e-10, 1.4e-12),
    "h2air:dense": (2.7e-13, 1.3e-10),
    "h2air:stiff": (1.4e-11, 4.1e-9),
    "h2air:sizes": (1.4e-10, 1.4e-12),
    "structured:unclipped": (2.9e-10, 1.4e-12),
    "structured:clipped": (4.6e-14, 6.4e-12),
    "structured:cool": (2.2e-10, 8.0e-13),
    "permuted:unclipped": (2.9e-10, 1.4e-12),
    "permuted:clipped": (1.1e-13, 3.0e-12),
    "permuted:cool": (2.2e-10, 9.1e-13),
    "frozen": (1.7e-10, 1.4e-12),
    "random:3,5": (9.6e-14, 9.1e-13),
    "random:10,17": (4.2e-10, 1.4e-12),
    "random:13,21": (4.7e-9, 2.6e-11),
    "random:16,40": (1.4e-12, 1.4e-12),
}
# mechanism: hiprtc compile wall time [s] (one core of the build machine)
COMPILE_S = {}
