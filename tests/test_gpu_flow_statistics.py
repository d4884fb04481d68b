"""Whole-field time averages on the device (hf2d_stats_tick / hf2d_stats_accum,
hip/flow_stats.hpp): every step's (p, T, rho, U, V) of each gas cell, read from
whichever representation is authoritative -- generic record, lean inviscid
arrays, lean N-S levels (SGL / SGT), lean mechanism state -- folded into
running weighted means, variances and the U-V covariance.

The oracle is NumPy (tests.test_flow_statistics.oracle) over the arrays of the
probe tests' recorder-free twin, which is advanced with step(1) and read with
field() and summary()["time"] after every step; every comparison is bitwise.
All runs start from tests.perturb.perturb with the autotune off.  Each case
asserts through the solver's counters that the kernel it names ran, and that
accumulating changed neither the counters nor the final fields."""
import functools

import numpy as np
import pytest

from openhyperflow2d_amd.models import decks
from openhyperflow2d_amd.models.simulation import PROBE_VARS
from tests.perturb import SCHEDULE, perturb
from tests.test_flow_statistics import assert_equals_oracle, oracle
from tests.test_gpu_probe_history import BIG, DECKS, GRAPH_SCHEDULE, SEED, _assert_path, _cells, _rows, _sim, _tile, _twin

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _solid(name):
    import openhyperflow2d_amd as hf

    a = np.asarray(_sim(hf, name, False).field("solid")).copy()
    a.setflags(write=False)
    return a


def _want(name, lo, hi, t0=0.0, **kw):
    times, fields = _twin(name)
    return oracle(times, fields, _solid(name), t0, lo, hi, **kw)


def _run(sim, sched):
    for n, res in sched:
        sim.step(n, residual=res)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("name", list(DECKS))
def test_averages_equal_the_oracle(gpu, monkeypatch, name, graphs):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    sched = GRAPH_SCHEDULE if graphs else SCHEDULE
    nsteps = sum(n for n, _ in sched)
    a, b = _sim(gpu, name, graphs), _sim(gpu, name, graphs)
    assert a.summary()["time"] == 0.0
    a.start_averaging()
    z = a.averages()
    assert z["samples"] == 0 and z["time"] == 0.0 and not z["mean"].any() and not z["var"].any()
    _run(a, sched)
    _run(b, sched)
    got = a.averages()
    solid = _solid(name)
    assert got["samples"] == nsteps and got["columns"] == (0, solid.shape[0])
    assert_equals_oracle(got, _want(name, 0, nsteps), what=name)
    for k in ("mean", "var"):
        assert not got[k][:, solid != 0.0].any(), k
    assert (got["var"][:, solid == 0.0] > 0).mean() > 0.5
    # the named kernel ran, and accumulating left neither the lean state nor the graphs
    T = _tile(gpu, name, *solid.shape)
    for s in (a, b):
        _assert_path(s.solver, name, T)
    assert (a.solver.graph_launches > 1) == graphs, a.solver.graph_launches
    for k in ("lns_steps", "lnm_steps", "graph_launches"):
        assert getattr(a.solver, k) == getattr(b.solver, k), k
    # reading the averages moved nothing: the next steps and the final fields are the plain run's
    sa, sb = a.summary(), b.summary()
    assert sa.keys() == sb.keys()
    for k in sa:
        np.testing.assert_array_equal(np.asarray(sa[k]), np.asarray(sb[k]), err_msg=k)   # (bitwise; NaN equals NaN)
    for f in PROBE_VARS + ("k", "CP"):
        np.testing.assert_array_equal(a.field(f), b.field(f), err_msg=f)


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_every_third_step_in_graphs(gpu, monkeypatch, name):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a = _sim(gpu, name, True)
    a.start_averaging(every=3)
    _run(a, GRAPH_SCHEDULE)
    assert a.solver.graph_launches > 1
    got = a.averages()
    assert got["samples"] == 13
    assert_equals_oracle(got, _want(name, 0, 40, every=3), what=name)


@pytest.mark.parametrize("name", ["wedge_tile", "scramjet_mech"])
def test_mean_only(gpu, monkeypatch, name):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a = _sim(gpu, name, True)
    a.start_averaging(second_moments=False)
    _run(a, GRAPH_SCHEDULE)
    got = a.averages()
    assert "var" not in got and "cov_uv" not in got
    assert_equals_oracle(got, _want(name, 0, 40, second_moments=False), what=name)
    np.testing.assert_array_equal(got["mean"], _want(name, 0, 40)["mean"])


@pytest.mark.parametrize("name", ["wedge_tile", "resonator_sgt"])
def test_arming_after_cached_windows(gpu, monkeypatch, name):
    """26 steps, arm, 26 more: exactly 26 samples, the twin's steps 27 .. 52.
    The windows cached before arming hold no accumulate node and must not
    replay (the arming generation in mode_signature)."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    n = 26
    a = _sim(gpu, name, True)
    a.step(n)
    before = a.solver.graph_launches
    assert before > 1
    a.start_averaging()
    a.step(n)
    times, _ = _twin(name)
    assert len(times) == 52
    got = a.averages()
    assert got["samples"] == n
    assert_equals_oracle(got, _want(name, n, 2 * n, t0=times[n - 1]), what=name)
    assert a.solver.graph_launches > before + 1   # captured again with the accumulator, then replayed


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_reset_and_stop_in_graphs(gpu, monkeypatch, name):
    """26 steps armed, reset, 14 more: the oracle over steps 27 .. 40 weighted
    from the reset; stopped, 12 further steps change nothing and the run is
    still the twin's."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a = _sim(gpu, name, True)
    with pytest.raises(RuntimeError):
        a.averages()
    with pytest.raises(ValueError):
        a.start_averaging(every=0)
    a.start_averaging()
    a.step(26)
    a.reset_averaging()
    z = a.averages()
    assert z["samples"] == 0 and z["time"] == 0.0 and not z["mean"].any() and not z["var"].any()
    a.step(14)
    times, fields = _twin(name)
    want = _want(name, 26, 40, t0=times[25])
    assert_equals_oracle(a.averages(), want, what="after reset")
    a.stop_averaging()
    a.step(12)
    assert_equals_oracle(a.averages(), want, what="stopped")
    assert a.summary()["time"] == times[51]
    np.testing.assert_array_equal(a.field("p"), fields["p"][51])


@pytest.mark.parametrize("name", ["wedge_flat", "step_split"])
def test_gpu_equals_cpu(gpu, monkeypatch, name):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    gen, kw, _, _ = DECKS[name]
    a = _sim(gpu, name, False)
    c = gpu.Simulation(gen(), "cpu", **kw)
    perturb(c, SEED)
    res = []
    for s in (a, c):
        s.start_averaging()
        _run(s, SCHEDULE)
        res.append(s.averages())
    g, h = res
    assert g["samples"] == h["samples"] == 14 and g["columns"] == h["columns"]
    assert g["time"] == h["time"]
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(g[k], h[k], err_msg=k)


@pytest.mark.parametrize("name", ["wedge_tile", "step_sgl"])
def test_download_and_upload_mid_run(gpu, monkeypatch, name):
    """download(); upload() after step 5 of 10 restarts the device's clock:
    the weights are still the twin's time differences, and no sample spans the
    upload."""
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    a, b = _sim(gpu, name, False), _sim(gpu, name, False)
    a.start_averaging()
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
    assert_equals_oracle(got, oracle(np.array(times), {v: np.array(x) for v, x in fields.items()}, _solid(name), 0.0),
                         what=name)
    assert (np.diff([0.0] + times) > 0).all()


@pytest.mark.parametrize("p2p", [False, True], ids=["local", "p2p"])
@pytest.mark.parametrize("deck", ["wedge", "step"])
def test_strips_accumulate_their_own_columns(gpu, monkeypatch, deck, p2p):
    """Three strips on virtual ranks: every rank's planes, placed by its
    `columns`, together are the one-GPU result; time and samples agree."""
    from openhyperflow2d_amd.parallel.strips import balanced_columns
    from tests.test_gpu_kernels import _virtual_ranks

    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    text = decks.wedge15(240, 60, **BIG) if deck == "wedge" else decks.step(240, 80, **BIG)
    ref = gpu.Simulation(text, "gpu")
    perturb(ref, SEED)
    solid = ref.field("solid")
    parts = balanced_columns(solid, 3)
    ref.start_averaging()
    _run(ref, SCHEDULE)
    one = ref.averages()
    held, stats = [], {}

    def setup(s):
        held.append(s)
        s.start_averaging(1, True, False)

    _virtual_ranks(gpu, text, 3, SCHEDULE, lean=True, p2p=p2p, setup=setup, parts=parts,
                   case_hook=lambda c: perturb(c, SEED), stats=stats)
    if deck == "step":
        assert min(stats["lns_steps"]) > 0 and ref.solver.lns_steps > 0, stats
    got = {k: np.full_like(one[k], np.nan) for k in ("mean", "var", "cov_uv")}
    for s, (a, b) in zip(held, parts):
        r = dict(s.averages())
        assert tuple(r["columns"]) == (a, b)
        assert int(r["samples"]) == one["samples"] == 14 and float(r["time"]) == one["time"]
        for k in got:
            got[k][..., a:b, :] = np.asarray(r[k])
    for k in got:
        np.testing.assert_array_equal(got[k], one[k], err_msg=k)


def test_coexists_with_the_probe_recorder(gpu, monkeypatch):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")
    name = "step_sgl"
    a = _sim(gpu, name, True)
    cells, _ = _cells(gpu, a, name)
    a.record_probes(cells, capacity=64)
    a.start_averaging()
    _run(a, GRAPH_SCHEDULE)
    assert a.solver.graph_launches > 1 and a.solver.lns_steps > 0
    times, fields = _twin(name)
    h = a.probe_history()
    assert h["total"] == 40
    np.testing.assert_array_equal(h["values"], _rows(fields, cells, 0, 40))
    np.testing.assert_array_equal(h["times"], times[:40])
    assert_equals_oracle(a.averages(), _want(name, 0, 40), what=name)
