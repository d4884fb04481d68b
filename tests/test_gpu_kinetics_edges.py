"""Every kinetics kernel on other mechanisms than H2/air and at the edges of
the state space (tests/kinetics_cases.py; its claims are checked on the CPU
in tests/test_kinetics_cases.py).

Standalone operators: the compiled hf2d_chem_fast (built-in mechanism only),
the hiprtc-specialised kernel, the MFMA kernel and the runtime-data VALU
kernel, against the host integrator mech_chem_host on every set and against
the NumPy oracle where its unclamped Newton applies.  Bounds: the project's
(1e-9 / 1e-8 K; 1e-7 / 1e-6 K on the random mechanisms), or ten times the
disagreement of the two FP64 CPU implementations where that is larger
(kinetics_cases.bound) -- none comes from a kernel's output.

Coupled step: hf2d_rtc_chem (compacted and dense), hf2d_chem_mech and
hf2d_chem_generic by DeviceSolver.chem_kernel on an 11-species reactor and on
a scramjet whose 16-cell tiles mix reacting and frozen cells."""
import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.ops import chemistry as ch
from openhyperflow2d_amd.ops import mechanism as M
from tests import kinetics_cases as K
from tests.test_chem_rtc import MECH, modified_mechanism
from tests.test_kinetics_cases import _converged, _oracle

pytestmark = pytest.mark.gpu

OPS = ("fast", "rtc", "mfma", "valu")
RUNTIME_OPS = OPS[1:]
EDGE_SETS = ("cold", "tmid", "far_guess", "clamped_guess", "no_radicals", "no_fuel", "bath_only", "negative", "thin",
             "dense", "stiff", "sizes")


def _run(nat, op, text, c):
    args = (c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub, 1)
    if op == "fast":
        return nat.chem_fast_run("h2_air_li2004", *args)[:2]
    if op == "rtc":
        return nat.chem_rtc_run(text, *args)[:2]
    return nat.chem_mech_run(text, *args, valu=op == "valu")[:2]


class _Lab:
    """Mechanisms, state sets and the CPU references, each computed once."""

    def __init__(self, nat):
        self.nat = nat
        self.li = M.h2_air_li2004()
        self.li_text = open(MECH).read()
        self.edges = K.edge_states(self.li)
        s = K.structured_mechanism()
        self.mech = {"structured": s, "permuted": K.permuted(s), "frozen": K.frozen_mechanism()}
        self.cases = {"structured": self._sets(s), "permuted": self._sets(self.mech["permuted"]),
                      "frozen": {"frozen": K.frozen_states(self.mech["frozen"])}}
        for ns, nr in K.RANDOM_SIZES:
            m, Y, rho, e, T = K.random_case(ns, nr)
            key = "random:%d,%d" % (ns, nr)
            self.mech[key] = m
            self.cases[key] = {key: [K.Case(Y, rho, e, T, dt, nsub) for dt, nsub in K.UNCLIPPED + [K.CLIPPED]]}
        self.text = {k: m.to_text() for k, m in self.mech.items()}
        # one hiprtc compile per mechanism (host side; the code objects are
        # cached on disk and the loaded modules in the process)
        self.rtc = {k: nat.chem_rtc_compile(t) for k, t in self.text.items()}
        self._host, self._np, self._dev = {}, {}, {}

    @staticmethod
    def _sets(m):
        return {"unclipped": K.structured_states(m, K.UNCLIPPED), "clipped": K.structured_states(m, [K.CLIPPED]),
                "cool": K.cool_states(m)}

    def host(self, key, text, c, k):
        if (key, k) not in self._host:
            self._host[key, k] = self.nat.mech_chem_host(text, c.rhoY, c.rho, c.e, c.T0, c.dt, c.nsub)
        return self._host[key, k]

    def oracle(self, key, m, c, k):
        if (key, k) not in self._np:
            self._np[key, k] = _oracle(m, c)
        return self._np[key, k]

    def device(self, op, key, text, c, k):
        if (op, key, k) not in self._dev:
            self._dev[op, key, k] = _run(self.nat, op, text, c)
        return self._dev[op, key, k]


@pytest.fixture(scope="module")
def lab(hf):
    return _Lab(hf.native())


def _check(got, Tg, ref, Tref, c, b, what, cells=slice(None)):
    ie = ch.increment_error(got[:, cells], ref[:, cells], c.rhoY[:, cells])
    dT = float(np.abs(Tg - Tref)[cells].max())
    print("%s: increment_error %.3g (bound %.2g)  |dT| %.3g K (bound %.2g)" % (what, ie, b[0], dT, b[1]))
    assert ie < b[0] and dT < b[1], what


def _check_mass(got, c):
    assert (np.abs(got.sum(0) - c.rho) <= 1e-12 * c.rho).all()


# ---------------------------------------------------------------------------
# H2/air at the state edges, all four kernels
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", EDGE_SETS)
def test_h2air_edge_states(gpu, lab, name, op):
    key = "h2air:" + name
    # far_guess / clamped_guess start from the solution of no set of the table:
    # the guess does not change the conditioning, the project bound holds
    b = K.bound(key) if key in K.TABLE else K.PROJECT_BOUND
    for k, c in enumerate(lab.edges[name]):
        ref, Tref = lab.host(key, "h2_air_li2004", c, k)
        got, Tg = lab.device(op, key, lab.li_text, c, k)
        assert np.isfinite(got).all() and np.isfinite(Tg).all()
        _check(got, Tg, ref, Tref, c, b, "%s %s[%d] against host" % (op, name, k))
        _check_mass(got, c)
        assert (got >= 0).all()
        if name == "bath_only":
            assert K.unchanged(got, c) and (got[:-1] == 0.0).all()
        if name in K.NEAR_GUESS or name == "cold":
            # the independent oracle: host's bound plus what host and oracle differ by
            orc, Torc = lab.oracle(key, lab.li, c, k)
            cells = _converged(lab.li, c, orc, Torc) if name == "cold" else slice(None)
            bn = tuple(x + y for x, y in zip(b, K.TABLE[key]))
            _check(got, Tg, orc, Torc, c, bn, "%s %s[%d] against NumPy" % (op, name, k), cells)


@pytest.mark.parametrize("name", EDGE_SETS)
def test_rtc_kernel_equals_compiled_kernel_on_edge_states(gpu, lab, name):
    """The generated struct and the shared kernel bodies through hiprtc == the
    kernel compiled into the library, bit for bit, at every edge."""
    key = "h2air:" + name
    for k, c in enumerate(lab.edges[name]):
        a, Ta = lab.device("fast", key, lab.li_text, c, k)
        b, Tb = lab.device("rtc", key, lab.li_text, c, k)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(Ta, Tb)


@pytest.mark.parametrize("op", OPS)
def test_prefix_of_the_cells_gives_the_prefix_of_the_result(gpu, lab, op):
    """n = 1 .. 257 (below one wavefront, one MFMA tile, one workgroup and
    across each): cells are independent, so on the same kernel every prefix
    reproduces the first n columns of the 257-cell result bit for bit."""
    cases = lab.edges["sizes"]
    full, Tfull = lab.device(op, "h2air:sizes", lab.li_text, cases[-1], len(cases) - 1)
    for k, c in enumerate(cases):
        got, Tg = lab.device(op, "h2air:sizes", lab.li_text, c, k)
        n = c.rho.size
        assert got.shape == (lab.li.ns, n)
        np.testing.assert_array_equal(got, full[:, :n], err_msg="n = %d" % n)
        np.testing.assert_array_equal(Tg, Tfull[:n], err_msg="n = %d" % n)


# ---------------------------------------------------------------------------
# other mechanisms through the runtime kernels
# ---------------------------------------------------------------------------
MECHS = ["structured", "permuted", "frozen"] + ["random:%d,%d" % s for s in K.RANDOM_SIZES]


@pytest.mark.parametrize("op", RUNTIME_OPS)
@pytest.mark.parametrize("mech", MECHS)
def test_runtime_kernels_on_other_mechanisms(gpu, lab, mech, op):
    m, text = lab.mech[mech], lab.text[mech]
    if op == "rtc":
        n, _, why = lab.rtc[mech]
        if m.nr == 0:
            # nothing to specialise: refused with a reason, on the host
            assert n < 0 and "without reactions" in why
            with pytest.raises(RuntimeError, match="without reactions"):
                _run(lab.nat, op, text, lab.cases[mech]["frozen"][0])   # (thrown on the host, nothing is launched)
            return
        assert n > 10000, why
    project = K.RANDOM_BOUND if mech.startswith("random") else K.PROJECT_BOUND
    for label, cases in lab.cases[mech].items():
        key = mech if label in (mech, "frozen") else mech + ":" + label
        b = K.bound(key, project)
        for k, c in enumerate(cases):
            ref, Tref = lab.host(key, text, c, k)
            got, Tg = lab.device(op, key, text, c, k)
            assert np.isfinite(got).all() and np.isfinite(Tg).all()
            _check(got, Tg, ref, Tref, c, b, "%s %s[%d] against host" % (op, key, k))
            _check_mass(got, c)
            if mech == "frozen":
                assert K.unchanged(got, c)
            if label != "clipped":
                orc, Torc = lab.oracle(key, m, c, k)
                bn = tuple(x + y for x, y in zip(b, K.TABLE[key]))
                _check(got, Tg, orc, Torc, c, bn, "%s %s[%d] against NumPy" % (op, key, k))


@pytest.mark.parametrize("op", RUNTIME_OPS)
def test_species_order_does_not_change_the_result(gpu, lab, op):
    """The structured mechanism with its species permuted (inerts last instead
    of first / in the middle / last): the result, un-permuted, is the
    original's within the host bound (the eliminations run in different
    orders, so not bit for bit)."""
    m, p = lab.mech["structured"], lab.mech["permuted"]
    ix = K.permutation(m, p)
    for label in ("unclipped", "clipped", "cool"):
        b = K.bound("structured:" + label)
        for k, (ca, cb) in enumerate(zip(lab.cases["structured"][label], lab.cases["permuted"][label])):
            ya, Ta = lab.device(op, "structured:" + label, lab.text["structured"], ca, k)
            yb, Tb = lab.device(op, "permuted:" + label, lab.text["permuted"], cb, k)
            _check(yb, Tb, ya[ix], Ta, cb, b, "%s permuted against original, %s[%d]" % (op, label, k))


# ---------------------------------------------------------------------------
# coupled step: every kernel of DeviceSolver.chem_kernel
# ---------------------------------------------------------------------------
KERNELS = [(4, True, "hf2d_rtc_chem"), (4, False, "hf2d_rtc_chem"), (2, True, "hf2d_chem_mech"),
           (3, True, "hf2d_chem_generic")]
FLOW = ("rho", "U", "V", "p", "T")


def _deck(which, path):
    if which == "reactor":
        return decks.with_mechanism(decks.reactor0d(8, 8, T=1200.0, p=101325.0), mechanism=path, substeps=2)
    return decks.with_mechanism(decks.scramjet(150, 50, nmax=10 ** 6, nout=10 ** 5), mechanism=path, substeps=2,
                                tmin=250.0)


def _advance(sim, which):
    if which == "reactor":
        sim.step(300)
    else:
        sim.step(40, residual=True)


@pytest.fixture(scope="module")
def coupled(hf, tmp_path_factory):
    """Deck text, species and the CPU result of the two coupled cases."""
    d = tmp_path_factory.mktemp("mech")
    out = {}
    for which, text, names in (("reactor", K.structured_mechanism().to_text(), K.STRUCTURED_ORDER),
                               ("scramjet", modified_mechanism(), M.h2_air_li2004().names)):
        path = d / (which + ".mech")
        path.write_text(text)
        deck = _deck(which, str(path))
        c = hf.Simulation(deck, "cpu")
        _advance(c, which)
        fields = FLOW + tuple("Y:" + s for s in names)
        out[which] = (deck, fields, {f: c.field(f).copy() for f in fields})
    return out


def _against_cpu(g, fields, cpu):
    for f in fields:
        a, b = g.field(f), cpu[f]
        tol = 1e-6 * b.max() if f == "T" else 1e-9 * max(np.abs(b).max(), 1e-30)
        assert np.abs(a - b).max() <= tol, f


@pytest.mark.parametrize("which", ["reactor", "scramjet"])
def test_coupled_step_on_every_kinetics_kernel(gpu, coupled, which):
    """reactor: 11 species (hf2d_chem_generic<MECH_MAXSP>, MFMA NSP = 12, AR
    from the air slot in every cell).  scramjet: a mechanism no compiled kernel
    covers at ChemTmin 250 K on 150 x 50: 16-cell MFMA tiles that are fully
    reacting, mixed (the frozen cells compute on a dummy state and must not
    store) and fully frozen."""
    deck, fields, cpu = coupled[which]
    if which == "reactor":
        assert cpu["Y:AR"].min() > 0.01 and cpu["Y:OH"].max() > 0.0
    else:
        # mixed tiles: reacting (T >= ChemTmin) and frozen cells side by side
        hot = (cpu["T"] >= 250.0).ravel()    # (cell index = i * ny + j)
        per_tile = hot[:hot.size // 16 * 16].reshape(-1, 16).sum(1)
        assert (per_tile == 16).sum() > 50 and (per_tile == 0).sum() > 50
        assert ((per_tile > 0) & (per_tile < 16)).sum() > 50
    rtc = {}
    for kind, compact, name in KERNELS:
        g = gpu.Simulation(deck, "gpu")
        assert not g.solver.chem_fast_ok and g.solver.chem_rtc_ok, g.solver.chem_rtc_why
        g.solver.chem_kernel = kind
        g.solver.chem_compact = compact
        _advance(g, which)
        assert g.solver.chem_kernel_used == name, (kind, compact)
        _against_cpu(g, fields, cpu)
        if kind == 4:
            rtc[compact] = {f: g.field(f).copy() for f in fields}
    for f in fields:   # compacted list of the reacting cells == one cell per lane
        np.testing.assert_array_equal(rtc[True][f], rtc[False][f], err_msg=f)


def test_mfma_kernel_on_a_strip_that_starts_off_a_tile_boundary(gpu, coupled):
    """Two strips of the scramjet on virtual ranks: the second strip's kinetics
    start at a ghost column of its local array, a multiple of ny = 50 cells
    and not of 16, so its MFMA tiles group other cells than the single-strip
    run's.  Cells are independent: bit for bit the single strip's result."""
    from tests.test_gpu_kernels import _virtual_ranks

    deck, fields, cpu = coupled["scramjet"]
    one = gpu.Simulation(deck, "gpu", lean=False)
    one.solver.chem_kernel = 2
    _advance(one, "scramjet")
    used = []

    def setup(s):
        s.chem_kernel = 2
        used.append(s)

    got, _ = _virtual_ranks(gpu, deck, 2, [(40, True)], lean=False, setup=setup, fields=fields)
    assert [s.chem_kernel_used for s in used] == ["hf2d_chem_mech"] * 2
    for f in fields:
        np.testing.assert_array_equal(got[f], one.field(f), err_msg=f)


def test_mechanism_without_reactions_in_the_coupled_step(gpu, tmp_path):
    """hiprtc refuses an empty reaction table with a reason; the kernel that
    takes the mechanism instead (MFMA: 16 null reactions; the generic kernel's
    reaction loop is empty) matches the CPU."""
    path = tmp_path / "frozen.mech"
    K.frozen_mechanism().save(str(path))
    deck = _deck("reactor", str(path))
    c = gpu.Simulation(deck, "cpu")
    c.step(300)
    fields = FLOW + tuple("Y:" + s for s in K.STRUCTURED_ORDER)
    cpu = {f: c.field(f).copy() for f in fields}
    for kind, name in ((0, "hf2d_chem_mech"), (3, "hf2d_chem_generic")):
        g = gpu.Simulation(deck, "gpu")
        assert not g.solver.chem_fast_ok
        assert not g.solver.chem_rtc_ok and "without reactions" in g.solver.chem_rtc_why
        g.solver.chem_kernel = kind
        g.step(300)
        assert g.solver.chem_kernel_used == name
        _against_cpu(g, fields, cpu)
        assert g.field("Y:OH").max() == 0.0 and g.field("Y:AR").min() > 0.01


def test_generic_kernel_on_the_builtin_mechanism(gpu):
    """chem_kernel = 3 on the built-in set: hf2d_chem_generic<9> through
    ignition (chem_fast = False selects the hiprtc kernel there)."""
    text = decks.with_mechanism(decks.reactor0d(8, 8, T=1200.0, p=101325.0), substeps=2)
    g = gpu.Simulation(text, "gpu")
    g.solver.chem_kernel = 3
    c = gpu.Simulation(text, "cpu")
    g.step(800)
    c.step(800)
    assert g.solver.chem_kernel_used == "hf2d_chem_generic"
    Tg, Tc = g.field("T"), c.field("T")
    assert Tc.max() > 2500.0   # ignited
    assert np.abs(Tg - Tc).max() < 1e-6 * Tc.max()
    for s in ("H2", "O2", "H2O", "OH", "H"):
        assert np.abs(g.field("Y:" + s) - c.field("Y:" + s)).max() < 1e-9, s
