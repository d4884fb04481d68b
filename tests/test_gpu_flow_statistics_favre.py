"""Favre averages and species statistics on the device (hf2d_stats_accum_x,
hip/flow_stats.hpp): with favre or species armed the cell pass also folds the
density-weighted T, U, V and the listed species' mass fractions rhoY_s / rho,
read from the species planes a download after the step would read, into their
own planes.

The oracle is NumPy (tests.test_flow_statistics_favre.oracle_x, and
tests.test_flow_statistics.oracle for the unchanged base keys) over a
recorder-free twin advanced with step(1) and read with field() and
summary()["time"] after every step; every comparison is bitwise.  All runs
start from tests.perturb.perturb with the autotune off.

Species run on scramjet(300, 23), the smallest grid on which the 2 mm injector
slot maps to cells (19 x 2 mechanism tiles with partial edge tiles; on
scramjet(37, 23) the H-bearing species are identically 0): the lean mechanism
step, the same with ChemTmin = 200 K so that every cell goes through the
kinetics list and hf2d_lnm_hot, and the split mechanism path.  Measured on the
CPU backend: each of the nine species has a positive variance in at least
11.5 % of the gas cells after the 14 steps of SCHEDULE and in at least 32 %
after the 40 of GRAPH_SCHEDULE (asserted: 5 % and 20 %)."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.perturb import SCHEDULE, perturb
from tests.test_flow_statistics import assert_equals_oracle, oracle
from tests.test_flow_statistics_favre import (H2_AIR, SUBSET, X_KEYS, assert_equals_oracle_x, assert_not_trivial,
                                              favre_vars, oracle_x)
from tests.test_gpu_probe_history import BIG, DECKS, GRAPH_SCHEDULE, SEED, _assert_path, _sim, _tile, _twin

pytestmark = pytest.mark.gpu

# species variants of scramjet(300, 23): (deck text, solver attributes, lean mechanism step)
SCRAMJET = {
    "lean": (lambda: decks.scramjet(300, 23, **BIG), {}, True),
    "hot": (lambda: decks.with_mechanism(decks.scramjet(300, 23, **BIG), tmin=200.0), {}, True),
    "split": (lambda: decks.scramjet(300, 23, **BIG), {"lean_mech": False}, False),
}
SJ_FIELDS = PROBE_VARS + tuple("Y:" + s for s in H2_AIR)


@functools.lru_cache(maxsize=None)
def _solid(name):
    import openhyperflow2d_amd as hf

    a = np.asarray(_sim(hf, name, False).field("solid")).copy()
    a.setflags(write=False)
    return a


def _run(sim, sched):
    for n, res in sched:
        sim.step(n, residual=res)


def _want(name, lo, hi, t0=0.0, **kw):
    """(extension, base) oracles of a DECKS path (Favre only: no species there)."""
    times, fields = _twin(name)
    base = {k: v for k, v in kw.items() if k in ("every", "second_moments", "weight")}
    return (oracle_x(times, fields, _solid(name), t0, lo, hi, favre=True, **kw),
            oracle(times, fields, _solid(name), t0, lo, hi, **base))


def _assert(got, want, what):
    assert_equals_oracle_x(got, want[0], what=what)
    assert_equals_oracle(got, want[1], what=what)


def _sj(gpu, variant, graphs):
    gen, attrs, _ = SCRAMJET[variant]
    s = gpu.Simulation(gen(), "gpu")
    perturb(s, SEED)
    for k, v in attrs.items():
        setattr(s.solver, k, v)
    s.solver.use_graph = graphs
    return s


@functools.lru_cache(maxsize=None)
def _sj_twin(variant, nsteps=40):
    """times [n], fields {name: [n, nx, ny]} (p, T, rho, U, V and Y:<s> of all
    nine species) and solid of the variant's recorder-free twin after each of
    its one-step calls (computed once, read-only)."""
    import openhyperflow2d_amd as hf

    s = _sj(hf, variant, False)
    assert tuple(s.case.mech_species) == H2_AIR
    solid = np.asarray(s.field("solid")).copy()
    times, fields = [], {v: [] for v in SJ_FIELDS}
    for _ in range(nsteps):
        s.step(1)
        s.solver.download()
        for v in SJ_FIELDS:
            fields[v].append(np.asarray(s.case.field(v)).copy())
        times.append(s.summary()["time"])
    out = {v: np.array(a) for v, a in fields.items()}
    for a in list(out.values()) + [solid]:
        a.setflags(write=False)
    return np.array(times), out, solid


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_favre_equals_the_oracle(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _sim(gpu, name, graphs), _sim(gpu, name, graphs)
    a.start_averaging(favre=True)
    z = a.averages()
    assert z["samples"] == 0 and not any(z[k].any() for k in X_KEYS if k in z)
    _run(a, sched)
    _run(b, sched)
    got = a.averages()
    solid = _solid(name)
    assert got["samples"] == nsteps and got["favre_vars"] == ("T", "U", "V") and "species" not in got
    _assert(got, _want(name, 0, nsteps), name)
    assert_not_trivial(got, solid, what=name)
    # the named kernel ran, and accumulating left neither the lean state nor the graphs
    T = _tile(gpu, name, *solid.shape)
    for s in (a, b):
        _assert_path(s.solver, name, T)
    assert (a.solver.graph_launches > 1) == graphs, a.solver.graph_launches
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(a.solver, k) == getattr(b.solver, k), k
    sa, sb = a.summary(), b.summary()
    for k in sa:
        np.testing.assert_array_equal(np.asarray(sa[k]), np.asarray(sb[k]), err_msg=k)   # (bitwise; NaN equals NaN)
    for f in PROBE_VARS + ("k", "CP"):
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("variant", list(SCRAMJET))
def test_species_and_favre_on_the_scramjet(gpu, monkeypatch, variant, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _sj(gpu, variant, graphs), _sj(gpu, variant, graphs)
    a.start_averaging(favre=True, species="all")
    _run(a, sched)
    _run(b, sched)
    got = a.averages()
    times, fields, solid = _sj_twin(variant)
    assert got["samples"] == nsteps and got["species"] == H2_AIR and got["favre_vars"] == favre_vars(H2_AIR)
    assert got["species_mean"].shape == (9,) + solid.shape and got["favre_mean"].shape == (12,) + solid.shape
    assert_equals_oracle_x(got, oracle_x(times, fields, solid, 0.0, 0, nsteps, favre=True, species=H2_AIR), what=variant)
    assert_equals_oracle(got, oracle(times, fields, solid, 0.0, 0, nsteps), what=variant)
    assert_not_trivial(got, solid, H2_AIR, species_share=0.2 if graphs else 0.05, what=variant)
    # the path the variant names ran, accumulating changed neither it nor the state
    lean = SCRAMJET[variant][2]
    for s in (a, b):
        assert (s.solver.lnm_steps > 0) == lean and s.solver.lns_steps == 0, (s.solver.lnm_steps, s.solver.lns_steps)
    assert (a.solver.graph_launches > 1) == graphs, a.solver.graph_launches
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(a.solver, k) == getattr(b.solver, k), k
    assert a.summary()["time"] == b.summary()["time"] == times[nsteps - 1]
    a.solver.download()
    b.solver.download()
    for f in SJ_FIELDS:
        np.testing.assert_array_equal(a.case.field(f), b.case.field(f), err_msg=f)
        np.testing.assert_array_equal(a.case.field(f), fields[f][nsteps - 1], err_msg=f)


@pytest.mark.parametrize("variant", ["lean", "split"])
def test_species_subset_in_list_order(gpu, monkeypatch, variant):
    """["OH", "H2", "N2"]: not the mechanism's order; without Favre, mean only
    on the split path."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    second = variant == "lean"
    a = _sj(gpu, variant, True)
    a.start_averaging(species=SUBSET, favre=second, second_moments=second)
    _run(a, GRAPH_SCHEDULE)
    got = a.averages()
    times, fields, solid = _sj_twin(variant)
    assert got["species"] == tuple(SUBSET) and ("favre_mean" in got) == second and ("species_var" in got) == second
    assert_equals_oracle_x(got, oracle_x(times, fields, solid, 0.0, 0, 40, favre=second, second_moments=second,
                                         species=SUBSET), what=variant)
    assert_equals_oracle(got, oracle(times, fields, solid, 0.0, 0, 40, second_moments=second), what=variant)
    assert_not_trivial(got, solid, SUBSET, species_share=0.2, what=variant)
    assert not np.array_equal(got["species_mean"][0], got["species_mean"][1])


def test_every_third_step_in_graphs(gpu, monkeypatch):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a = _sim(gpu, "wedge_tile", True)
    a.start_averaging(every=3, favre=True)
    _run(a, GRAPH_SCHEDULE)
    assert a.solver.graph_launches > 1
    got = a.averages()
    assert got["samples"] == 13
    _assert(got, _want("wedge_tile", 0, 40, every=3), "wedge_tile")
    s = _sj(gpu, "lean", True)
    s.start_averaging(every=3, weight="step", favre=True, species="all")
    _run(s, GRAPH_SCHEDULE)
    assert s.solver.graph_launches > 1 and s.solver.lnm_steps > 0
    got = s.averages()
    times, fields, solid = _sj_twin("lean")
    kw = dict(every=3, weight="step")
    assert got["samples"] == 13
    assert_equals_oracle_x(got, oracle_x(times, fields, solid, 0.0, 0, 40, favre=True, species=H2_AIR, **kw))
    assert_equals_oracle(got, oracle(times, fields, solid, 0.0, 0, 40, **kw))


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_arming_after_cached_windows(gpu, monkeypatch, name):
    """26 steps, arm, 26 more: exactly 26 samples, the twin's steps 27 .. 52."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    n = 26
    a = _sim(gpu, name, True)
    a.step(n)
    before = a.solver.graph_launches
    assert before > 1
    a.start_averaging(favre=True)
    a.step(n)
    times, _ = _twin(name)
    got = a.averages()
    assert got["samples"] == n
    _assert(got, _want(name, n, 2 * n, t0=times[n - 1]), name)
    assert a.solver.graph_launches > before + 1   # captured again with the accumulator, then replayed


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_reset_stop_and_fewer_options_in_graphs(gpu, monkeypatch, name):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a = _sim(gpu, name, True)
    with pytest.raises(ValueError):
        a.start_averaging(favre=True, species="all")   # not a mechanism deck
    with pytest.raises(RuntimeError):
        a.averages()
    a.start_averaging(favre=True)
    a.step(26)
    a.reset_averaging()
    z = a.averages()
    assert z["samples"] == 0 and z["time"] == 0.0 and not any(z[k].any() for k in X_KEYS if k in z)
    a.step(14)
    times, fields = _twin(name)
    want = _want(name, 26, 40, t0=times[25])
    _assert(a.averages(), want, "after reset")
    a.stop_averaging()
    a.step(6)
    _assert(a.averages(), want, "stopped")
    # armed again without the option: the base kernel and keys, planes reused
    a.start_averaging()
    a.step(6)
    got = a.averages()
    assert "favre_mean" not in got and "favre_vars" not in got
    assert_equals_oracle(got, oracle(times, fields, _solid(name), times[45], 46, 52), what="armed again")
    assert a.summary()["time"] == times[51]
    np.testing.assert_array_equal(a.field("p"), fields["p"][51])


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_download_and_upload_mid_run(gpu, monkeypatch, name):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a, b = _sim(gpu, name, False), _sim(gpu, name, False)
    a.start_averaging(favre=True)
    times, fields = [], {v: [] for v in PROBE_VARS}
    for k in range(10):
        b.step(1)
        for v in PROBE_VARS:
            fields[v].append(b.field(v).copy())
        times.append(b.summary()["time"])
        if k == 4:
            b.solver.download()
            b.solver.upload()
    a.step(5)
    a.solver.download()
    a.solver.upload()
    a.step(5)
    got = a.averages()
    assert got["samples"] == 10
    times, fields = np.array(times), {v: np.array(x) for v, x in fields.items()}
    assert_equals_oracle_x(got, oracle_x(times, fields, _solid(name), 0.0, favre=True), what=name)
    assert_equals_oracle(got, oracle(times, fields, _solid(name), 0.0), what=name)


def test_download_and_upload_mid_run_species(gpu, monkeypatch):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a, b = _sj(gpu, "lean", False), _sj(gpu, "lean", False)
    a.start_averaging(favre=True, species=SUBSET)
    times, fields = [], {v: [] for v in SJ_FIELDS}
    for k in range(8):
        b.step(1)
        b.solver.download()
        for v in SJ_FIELDS:
            fields[v].append(np.asarray(b.case.field(v)).copy())
        times.append(b.summary()["time"])
        if k == 3:
            b.solver.upload()
    a.step(4)
    a.solver.download()
    a.solver.upload()
    a.step(4)
    got = a.averages()
    assert got["samples"] == 8 and a.solver.lnm_steps > 0
    times, fields = np.array(times), {v: np.array(x) for v, x in fields.items()}
    solid = _sj_twin("lean")[2]
    assert_equals_oracle_x(got, oracle_x(times, fields, solid, 0.0, favre=True, species=SUBSET))
    assert_equals_oracle(got, oracle(times, fields, solid, 0.0))


def test_strips_accumulate_their_own_columns(gpu, monkeypatch):
    """Three strips on virtual ranks (local transport): every rank's planes,
    placed by its `columns`, together are the one-GPU result."""
    from openhyperflow2d_amd.parallel.strips import balanced_columns
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(240, 60, **BIG)
    ref = gpu.Simulation(text, "gpu")
    perturb(ref, SEED)
    parts = balanced_columns(ref.field("solid"), 3)
    ref.start_averaging(favre=True)
    _run(ref, SCHEDULE)
    one = ref.averages()
    held = []

    def setup(s):
        held.append(s)
        s.start_averaging(1, True, False, True)

    _virtual_ranks(gpu, text, 3, SCHEDULE, lean=True, p2p=False, setup=setup, parts=parts,
                   case_hook=lambda c: perturb(c, SEED), stats={})
    keys = ("mean", "var", "cov_uv") + tuple(k for k in X_KEYS if k.startswith("favre"))
    got = {k: np.full_like(one[k], np.nan) for k in keys}
    for s, (a, b) in zip(held, parts):
        r = dict(s.averages())
        assert tuple(r["columns"]) == (a, b)
        assert int(r["samples"]) == one["samples"] == 14 and float(r["time"]) == one["time"]
        for k in got:
            got[k][..., a:b, :] = np.asarray(r[k])
    for k in got:
        np.testing.assert_array_equal(got[k], one[k], err_msg=k)
    assert (one["favre_weight"][np.asarray(ref.field("solid")) == 0.0] > 0).all()


@pytest.mark.parametrize("name", ["wedge_flat", "step_split"])
def test_gpu_equals_cpu(gpu, monkeypatch, name):
    """Favre only: the mechanism kinetics agree to 1e-9 between the backends, not bitwise."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    gen, kw, _, _ = DECKS[name]
    a = _sim(gpu, name, False)
    c = gpu.Simulation(gen(), "cpu", **kw)
    perturb(c, SEED)
    res = []
    for s in (a, c):
        s.start_averaging(favre=True)
        _run(s, SCHEDULE)
        res.append(s.averages())
    g, h = res
    assert g["samples"] == h["samples"] == 14 and g["time"] == h["time"]
    for k in ("mean", "var", "cov_uv") + tuple(k for k in X_KEYS if k.startswith("favre")):
        np.testing.assert_array_equal(g[k], h[k], err_msg=k)
