"""The FP32 GPU kernels cell for cell against the FP32 CPU stepper
(tests/fp32_cases.py: protocol, rules, rows; tests/test_fp32_cases.py: the
harness's own evidence on the CPU).

A. one process of bin/hf2d_fp32 on every stepper path against
   `hf2d_fp32 --backend cpu`, which path ran asserted from the profile's
   "path" object;
B. GPU against GPU: lean N-S == split, step graphs == eager, byte for byte;
C. 3 and 4 native processes through the mailboxes == one process, byte for
   byte (the float p2p_load / p2p_store overloads, float halo columns beside
   double dt words, the fused push and ghost prologue of the lean N-S tiles).

Every GPU process runs under its own time limit; after one that ends in a
time limit, an abort, a segmentation fault or a HIP fault message no further
GPU process is started and every later test fails at once."""
import functools

import pytest

from tests import fp32_cases as C

pytestmark = pytest.mark.gpu

_STOP = []   # why no further GPU process may start


@functools.lru_cache(maxsize=None)
def _gpu(deck, nmax, env, ranks):
    if _STOP:
        pytest.fail("no GPU process after " + _STOP[0])
    run = C.march(C.seed_of(deck, nmax), C.GPU_FP32, "gpu", ranks=ranks, env=dict(env))
    if C.faulted(run):
        _STOP.append("%s %r on %d rank(s): exit %d\n%s\n%s" % (deck, env, ranks, run.returncode, run.stdout[-1500:],
                                                              run.stderr[-1500:]))
        pytest.fail(_STOP[0])
    C.finished(run)
    for p in run.profile:
        assert p["path"]["fp"] == 32, p["path"]
    return run


def gpu_run(deck, nmax=C.NMAX, env=None, ranks=1):
    """One run per (deck, Nmax, environment, ranks) and session, shared."""
    return _gpu(deck, nmax, tuple(sorted((env or {}).items())), ranks)


def _figures(row, dist, scale):
    m = C.MEASURED.get(row.id, {})
    lines = ["%s (%s, %r): relative to the field's max over gas" % (row.id, row.deck, row.env),
             "%-8s %12s %12s %12s %12s" % ("field", "now", "recorded", "bound", "D")]
    for f in C.FIELDS:
        rec = m.get(f)
        lines.append("%-8s %12.3e %12s %12s %12.3e" % (f, dist[f], "-" if rec is None else "%.3e" % rec,
                                                      "-" if rec is None else "%.3e" % (4 * rec), scale[f]))
    return "\n".join(lines)


@pytest.mark.parametrize("row_id", [r.id for r in C.ROWS])
def test_gpu_fp32_equals_cpu_fp32(gpu, row_id, capsys):
    """Section A."""
    row = C.BY_ID[row_id]
    ref = C.cpu_reference(row.deck, row.nmax)
    run = gpu_run(row.deck, row.nmax, row.env)
    bad = C.facts_missed(row, run)
    assert not bad, "; ".join(bad)
    dist, masks = C.distances(run, ref)
    rule = C.rule_of(row)
    if row.rule == "measured":
        scale = C.precision_scale()[row.deck]
        text = _figures(row, dist, scale)
        with capsys.disabled():
            print("\n" + text)
        assert rule != "unmeasured", "no recorded figures for this row yet:\n" + text
    if rule == "equal values":   # a measured row whose named fields all recorded 0 (fp32_cases.MEASURED)
        bad = ["%s: %.3e, recorded 0" % (f, d) for f, d in dist.items() if d] + ["%s: non-finite mask" % f for f in masks]
        loose = C.UNNAMED.get(row.id, {})
        bad += C.equal_misses(run, ref, zero_signs=False, skip=tuple(loose))
        for name, recorded in loose.items():
            d = C.record_distance(run, ref, name)
            with capsys.disabled():
                print("%s %s: %.3e now, recorded %r" % (row.id, name, d, recorded))
            if recorded is None or not d <= 4.0 * recorded:
                bad.append("%s: %.3e against 4 x the recorded %r" % (name, d, recorded))
        assert not bad, "; ".join(bad)
        return
    if rule == "equal":
        bad = C.equal_misses(run, ref)
        assert not bad, "; ".join(bad) + "\nrelative to the field's max over gas: %s" % {
            f: "%.2e" % d for f, d in dist.items() if d}
        return
    assert not masks, "non-finite values in other cells than the reference's: %s" % masks
    recorded = C.MEASURED[row.id]
    assert sorted(recorded) == sorted(C.FIELDS)
    bad = []
    for f in C.FIELDS:
        bound = 4.0 * recorded[f]
        if not bound <= scale[f] / 4.0:
            bad.append("%s: bound %.3e above D / 4 = %.3e" % (f, bound, scale[f] / 4.0))
        if not dist[f] <= bound:
            bad.append("%s: %.3e above the bound %.3e" % (f, dist[f], bound))
    assert not bad, "; ".join(bad) + "\n" + text


def _same_bytes(a, b):
    bad = ([] if a.hf2d == b.hf2d else C.equal_misses(a, b) or [".hf2d: non-finite payloads differ"])
    bad += C.plt_misses(a, b)
    assert not bad, "; ".join(bad)


@pytest.mark.parametrize("deck", ["step_37x23", "resonator_37x23"])
def test_lean_ns_equals_split_in_float(gpu, deck):
    """Section B: the float twin of test_lean_ns_equals_split (laminar and
    k-eps), on the files."""
    lean, split = gpu_run(deck), gpu_run(deck, env={"LEAN_NS": 0})
    assert lean.profile[0]["path"]["lns_steps"] > 0 and split.profile[0]["path"]["lns_steps"] == 0
    _same_bytes(lean, split)


@pytest.mark.parametrize("row_id", ["headline_two_cell_graphs", "laminar_lean_ns"])
def test_step_graphs_equal_eager_in_float(gpu, row_id):
    """Section B: 6-step windows captured and replayed against eager steps."""
    row = C.BY_ID[row_id]
    env = dict(row.env)
    env.pop("GRAPH", None)
    on = gpu_run(row.deck, C.NMAX_GRAPH, dict(env, GRAPH=1))
    off = gpu_run(row.deck, C.NMAX_GRAPH, dict(env, GRAPH=0))
    assert on.profile[0]["path"]["graph_launches"] > 1 and on.profile[0]["path"]["graph_captures"] >= 1
    assert off.profile[0]["path"]["graph_launches"] == 0 and off.profile[0]["path"]["graph_captures"] == 0
    bad = C.facts_missed(row._replace(facts=[f for f in row.facts if "graphs" not in f[0]]), off)
    assert not bad, "; ".join(bad)
    _same_bytes(on, off)


# (deck, ranks, what every rank's profile must show)
STRIPS = [(deck, ranks) for deck in ("wedge_96x24", "resonator_96x24", "triple_96x24", "wedge_keps_96x24")
          for ranks in (3, 4)] + [("wedge_96x24_lagged", 4)]
STRIP_FACTS = {
    "wedge_96x24": ("the tile kernel with the fused exchange", lambda p: p["lean_tile_last"]["fx"] == 1),
    "wedge_96x24_lagged": ("the tile kernel with the fused exchange", lambda p: p["lean_tile_last"]["fx"] == 1),
    "resonator_96x24": ("the lean N-S tiles", lambda p: p["lns_steps"] > 0),
    "triple_96x24": ("the mixture lean kernels", lambda p: p["lean_ok"] is True and p["lean_sg_ok"] is False),
    "wedge_keps_96x24": ("split SK_SGT", lambda p: p["sk_mode"] == 2 and p["lns_steps"] == 0),
}
INVISCID_STRIP_DECKS = ("wedge_96x24", "wedge_96x24_lagged", "triple_96x24")


@pytest.mark.parametrize("deck,ranks", STRIPS)
def test_float_strips_through_the_mailboxes_equal_one_process(gpu, deck, ranks):
    """Section C."""
    one = gpu_run(deck)
    assert one.profile[0]["path"]["transport"] == "none"
    if deck in INVISCID_STRIP_DECKS:   # (with section A: strips == CPU)
        bad = C.equal_misses(one, C.cpu_reference(deck))
        assert not bad, "; ".join(bad)
    port = 29900 + 10 * STRIPS.index((deck, ranks))
    run = gpu_run(deck, env={"MASTER_PORT": port}, ranks=ranks)
    assert "halo transport p2p" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    assert "using RCCL" not in run.stdout + run.stderr, run.stderr[-2000:]
    what, pred = STRIP_FACTS[deck]
    for q, prof in enumerate(run.profile):
        p = prof["path"]
        assert (prof["rank"], prof["ranks"]) == (q, ranks)
        assert p["transport"] == "p2p", p
        assert pred(p), "rank %d did not run %s: %r" % (q, what, p)
    _same_bytes(run, one)
