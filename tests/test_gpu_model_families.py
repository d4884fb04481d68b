"""The GPU step on every turbulence-model family, contour and source deck of
tests/fixtures/ref, across a cycle boundary, against the plain per-cell CPU
stepper (table, protocol and comparison rules: tests/model_families.py).

run() ends in DeviceSolver::cycle_update(): lns_materialize(), hf2d_wall_uw,
the host merge and hf2d_yplus; the steps after it are the first in the suite
whose eddy viscosity reads a y+ computed on the device.  Every path asserts
which kernels ran (sk_mode / sgl_why, lean_ok / lean_tile_last, lns_ok /
lns_why / lns_turb / lns_steps), so a silent fall-back cannot pass; the CPU
reference's own conditions are test_model_family_decks.py.

Measured on an MI355X (largest difference over the four calls, relative to the
field's max): see the figures each test prints before it asserts."""
import pytest

from tests import model_families as mf

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_autotune(monkeypatch):
    monkeypatch.setenv("HF2D_AUTOTUNE", "0")


def _compare_every_call(g, row, tmp_path, after_call):
    """The schedule on g; after every call the path's own assertions, then the
    comparison.  The march goes on after a miss, so that the failure names
    the first call and every field that differs, call by call."""
    ref = mf.cpu_reference(row.id)
    worst, bad = {}, []
    for q in mf.march(g, tmp_path):
        after_call(q)
        figs, miss = mf.misses(row, g.field, g.summary(), ref.snaps[q], ref.gas)
        bad += ["call %d: %s" % (q, m) for m in miss]
        for f, d in figs.items():
            worst[f] = max(worst.get(f, 0.0), d)
    print("%s worst: %s" % (row.id, " ".join("%s=%.2e" % kv for kv in worst.items())))
    assert not bad, "\n".join(bad)


def _viscous_facts(sv):
    """What construction must find for every viscous row: single gas with a
    turbulence model (SK_SGT), nothing for the inviscid lean kernels."""
    assert (sv.sk_mode, sv.sgl_ok, sv.sgl_why) == (mf.SK_SGT, True, "turbulent: SK_SGT")
    assert (sv.lean_ok, sv.lean_why) == (False, "viscous problem")


@pytest.mark.parametrize("path", ["default", "generic"])
@pytest.mark.parametrize("rid", [r.id for r in mf.VISCOUS])
def test_viscous_family_across_a_cycle_matches_cpu(gpu, tmp_path, rid, path):
    """hf2d_predict / hf2d_fill<SK_SGT> (default) and <SK_GENERIC> (sgl =
    lean_ns = False), hf2d_wall_solid / hf2d_wall_wall, and hf2d_wall_uw /
    hf2d_yplus at the cycle boundary: NS_FIELDS to 1e-9 after every call.
    (cycle_update() once queued the upload of the merged friction velocities
    from host vectors it freed before the stream had run: on a loaded card
    y_plus of klebanoff stayed 0 over the whole field in one run of this test.)"""
    row = mf.BY_ID[rid]
    g = mf.simulation(gpu, row, "gpu")
    sv = g.solver
    _viscous_facts(sv)
    # wall heat transfer rules the lean N-S tiles out whatever the model
    assert (sv.lns_ok, sv.lns_why) == (False, "wall heat transfer")
    assert sv.sgl and sv.lean_ns
    if path == "generic":
        sv.sgl = False
        sv.lean_ns = False

    def after_call(q):
        assert sv.sgl == (path == "default")
        assert sv.lns_steps == 0 and sv.lnm_steps == 0
        assert sv.lean_tile_last["nt"] == 0, sv.lean_tile_last

    _compare_every_call(g, row, tmp_path, after_call)


@pytest.mark.parametrize("path", ["default", "generic"])
@pytest.mark.parametrize("rid", [r.id for r in mf.INVISCID])
def test_inviscid_deck_across_a_cycle_matches_cpu(gpu, tmp_path, rid, path):
    """The lean tile kernels (or, for a deck that is not lean-eligible, the
    fused Euler kernel) and the split predict / fill<SK_GENERIC> pair (lean =
    fused = False): == the CPU stepper bit for bit (zeldovich_reacting: 1e-9,
    its rate goes through device exp / pow)."""
    row = mf.BY_ID[rid]
    kw = {} if path == "default" else dict(lean=False, fused=False)
    g = mf.simulation(gpu, row, "gpu", **kw)
    sv = g.solver
    assert (sv.sk_mode, sv.sgl_ok, sv.sgl_why) == (mf.SK_GENERIC, False, "inviscid problem")
    assert (sv.lean_ok, sv.lean_why) == (row.lean_why == "", row.lean_why)
    assert (sv.lean, sv.fused) == ((True, True) if path == "default" else (False, False))
    tiles = path == "default" and sv.lean_ok

    def after_call(q):
        # (every call has at least three steps: all but a call's first run the tile kernel)
        assert (sv.lean_tile_last["nt"] != 0) == tiles, sv.lean_tile_last
        assert sv.lns_steps == 0 and sv.lnm_steps == 0

    _compare_every_call(g, row, tmp_path, after_call)


def test_recorder_and_averages_across_a_cycle_match_cpu(gpu, tmp_path):
    """DeviceSolver::on_cycle_roll() restarts the device's time_part with the
    host's cur_time_part (that is what makes `time` above == the CPU's after
    the boundary) and moves the two clocks derived from it: the probe
    recorder's stored times and the accumulator's offset.  Recorder and
    accumulator armed before run(): the averages and every row of the steps
    after the boundary equal the CPU's bit for bit; a row of the cycle before
    it is converted as global_time + (t_row - t_roll), two roundings of at
    most half an ulp of the boundary's time each."""
    import numpy as np

    row = mf.BY_ID["bff_linear"]
    g, c = mf.simulation(gpu, row, "gpu"), mf.simulation(gpu, row, "cpu", lean=False)
    cells = [(3, 2), (60, 20), (117, 37)]
    out = []
    for s in (g, c):
        assert all(s.field("solid")[i, j] == 0.0 for i, j in cells)
        s.record_probes(cells, capacity=64)
        s.start_averaging()
        assert list(mf.march(s, tmp_path)) == [0, 1, 2, 3]
        out.append((s.probe_history(), s.averages(), s.summary()))
    (hg, ag, sg), (hc, ac, sc) = out
    assert sg["time"] == sc["time"] and sg["iteration"] == sc["iteration"] == 43
    assert hg["total"] == hc["total"] == 43
    np.testing.assert_array_equal(hg["values"], hc["values"])
    np.testing.assert_array_equal(hg["times"][30:], hc["times"][30:])
    assert hg["times"][-1] == sg["time"]
    t_roll = hc["times"][29]
    assert np.abs(hg["times"][:30] - hc["times"][:30]).max() <= np.spacing(t_roll)
    assert (np.diff(hg["times"]) > 0).all()
    assert ag["samples"] == ac["samples"] == 43
    assert ag["time"] == ac["time"]
    for k in ("mean", "var", "cov_uv"):
        np.testing.assert_array_equal(ag[k], ac[k], err_msg=k)


def test_load_heat_and_surface_recorders_across_a_cycle_match_cpu(gpu, tmp_path):
    """The same roll for the three recorders that carry a plan: the load ring's
    times, the wall heat and surface rings' times, their peak times and the
    offsets of their weights' clocks all move by the device's time_part at the
    boundary.  All five observers armed before run() on the k-eps deck with wall
    heat transfer (split SK_SGT kernels), cycle boundary after step 30 of 43.

    On the GPU alone, bit for bit: one clock (every history's times are the
    probe history's, strictly increasing, ending at summary()["time"]), every
    peak time is one of those times, and the three weight sums are one number.
    A block of the roll that shifts by another amount or misses an array breaks
    one of the three.  Against the CPU recorders: the row's rule, REL of the
    CPU array's largest magnitude."""
    import numpy as np

    from tests.test_gpu_load_history import targets

    row = mf.BY_ID["monitors_heatflux_cx"]
    g, c = mf.simulation(gpu, row, "gpu"), mf.simulation(gpu, row, "cpu", lean=False)
    _viscous_facts(g.solver)
    cells = [(3, 2), (60, 20), (117, 37)]
    out = []
    for s in (g, c):
        assert all(s.field("solid")[i, j] == 0.0 for i, j in cells)
        s.record_probes(cells, capacity=64)
        s.start_averaging()
        s.record_loads(*targets(s.case), capacity=64)
        s.record_wall_heat(capacity=64)
        s.record_surface(capacity=64)
        assert list(mf.march(s, tmp_path)) == [0, 1, 2, 3]
        out.append((s.probe_history(), s.averages(), s.load_history(), s.wall_heat_history(), s.surface_history(),
                    s.summary()))
    (pg, ag, lg, wg, fg, sg), (pc, ac, lc, wc, fc, sc) = out
    assert sg["iteration"] == sc["iteration"] == 43
    for h in (pg, lg, wg, fg, pc, lc, wc, fc):
        assert h["total"] == 43
    for h in (ag, wg, fg, ac, wc, fc):
        assert h["samples"] == 43

    # the CPU twin: what the deck gives the recorders, and none of it constant
    assert (int(wc["x_nodes"].sum()), int(wc["y_nodes"].sum()), len(fc["i"])) == (80, 83, 84)
    assert ((fc["fric_x"] != 0) | (fc["fric_y"] != 0)).all()   # (every surface node has a friction term)
    twin = {"forces": lc["forces"], "mass_flow": lc["mass_flow"], "x": wc["x"], "y": wc["y"], "values": fc["values"]}
    for k, a in twin.items():
        assert np.isfinite(a).all() and a.shape[0] == 43, k
        assert (a.reshape(43, -1).max(axis=0) > a.reshape(43, -1).min(axis=0)).any(), k + " is constant"
    t_roll = pc["times"][29]
    assert (fc["peak_time"] <= t_roll).any() and (fc["peak_time"] > t_roll).any()

    # one clock on the device
    times = pg["times"]
    for name, h in (("loads", lg), ("wall heat", wg), ("surface", fg)):
        np.testing.assert_array_equal(h["times"], times, err_msg=name)
    assert (np.diff(times) > 0).all() and times[-1] == sg["time"]
    for name, pt in (("surface", fg["peak_time"]), ("wall heat x", wg["peak_time_x"]), ("wall heat y", wg["peak_time_y"])):
        stray = ~np.isin(pt, times)
        assert not stray.any(), "%s: %d peak times are no sample's time, e.g. %r" % (name, stray.sum(), pt[stray][:3])
    assert (fg["peak_time"] <= times[29]).any() and (fg["peak_time"] > times[29]).any()
    assert wg["time"] == fg["time"] == ag["time"], (wg["time"], fg["time"], ag["time"])

    # against the CPU recorders
    pairs = [("forces", lg["forces"], lc["forces"]), ("mass_flow", lg["mass_flow"], lc["mass_flow"]),
             ("loads times", lg["times"], lc["times"])]
    pairs += [("wall heat " + k, wg[k], wc[k]) for k in ("x", "y", "mean_x", "mean_y", "peak_x", "peak_y", "times", "time")]
    pairs += [("surface " + k, fg[k], fc[k]) for k in ("values", "mean", "peak", "times", "time")]
    pairs += [("probe times", pg["times"], pc["times"]), ("averages time", ag["time"], ac["time"])]
    bad = []
    for name, x, y in pairs:
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        assert x.shape == y.shape, name
        top, d = float(np.abs(y).max()), float(np.abs(x - y).max())
        print("%s: max |gpu - cpu| %.3e, max |cpu| %.6e" % (name, d, top))
        if not d <= mf.REL * top:   # (a NaN misses)
            bad.append("%s: max |diff| %.3e > %.1e * %.6e" % (name, d, mf.REL, top))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("rid", [r.id for r in mf.LNS])
def test_lean_ns_tiles_across_a_cycle_match_cpu(gpu, tmp_path, rid):
    """hf2d_lns_step<SK_SGT, k-eps | Spalart-Allmaras> through the cycle
    boundary: lns_materialize() in cycle_update(), y+ on the materialised
    record, and the lean re-entry in the steps after it.  lns_steps must have
    grown both in the run() call (before the boundary) and in the calls after
    it.  Chien's k-eps must be refused and run the split kernels."""
    row = mf.BY_ID[rid]
    g = mf.simulation(gpu, row, "gpu")
    sv = g.solver
    _viscous_facts(sv)
    assert sv.sgl and sv.lean_ns
    if row.lns_why:
        assert (sv.lns_ok, sv.lns_why) == (False, row.lns_why)
    else:
        assert sv.lns_ok, sv.lns_why
        assert sv.lns_turb == row.lns_turb
    assert sv.lns_steps == 0
    seen = []

    def after_call(q):
        seen.append(sv.lns_steps)
        assert sv.lean_tile_last["nt"] == 0, sv.lean_tile_last
        if row.lns_why:
            assert sv.lns_steps == 0
        else:
            # (a call's first step is the split entry step: the comparison before it
            # downloaded, i.e. materialised; every later step of the call is a lean one)
            assert sv.lns_steps > (seen[-2] if q else 0), seen

    _compare_every_call(g, row, tmp_path, after_call)
    assert len(seen) == 4
