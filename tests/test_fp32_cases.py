"""The claims tests/fp32_cases.py makes, checked on the CPU: the record dtypes
parse a real checkpoint; the float CPU stepper inside bin/hf2d_fp32 (hipcc's
host compiler) writes what the g++ build bin/hf2d_cpu_fp32 writes, so it is a
reference and not a third implementation; it is strip-independent; and the
precision yardstick D of the "close" rule, the distance between the FP32 and
the FP64 CPU stepper, is a usable scale."""
import json
import os

import numpy as np
import pytest

from tests import fp32_cases as C


@pytest.fixture(scope="module")
def cpu_fp32(hf):
    from openhyperflow2d_amd import _build

    exe = _build.build_fp32()
    assert os.path.samefile(exe, C.CPU_FP32)
    return exe


def test_record_dtypes_have_the_struct_sizes():
    assert C.REC32.itemsize == 680 and C.REC64.itemsize == 1248
    # the offsets core/common.hpp pins for the FP64 record
    want = {"TurbType": 216, "x": 296, "p": 352, "CT": 384, "beta": 400, "A": 544, "Tg": 1048, "Y": 1072,
            "droYdx": 1120, "dUdx": 1184, "BGX": 1232}
    assert {n: C.REC64.fields[n][1] for n in want} == want


@pytest.mark.parametrize("exe", ["GPU_FP32", "CPU_FP64"])
def test_record_dtypes_parse_a_checkpoint(hf, exe):
    """x, y sit behind the padded TurbType word and nine more reals: every
    record's equal the grid's cell centres, in both layouts."""
    deck = "wedge_37x23"
    run = C.cpu_reference(deck) if exe == "GPU_FP32" else C.finished(
        C.march(C.seed_of(deck, C.NMAX, C.CPU_FP64), C.CPU_FP64, "cpu"))
    nx, ny = run.grid
    assert (nx, ny) == (37, 23)
    rec = run.records.reshape(nx, ny)
    assert rec.dtype == (C.REC32 if exe == "GPU_FP32" else C.REC64)
    i, j = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    # (the pre-processor leaves ix, iy and the neighbour pointers 0, as the reference's does: the
    # words between y and p hold nothing but zeros, and p, which follows them, is a pressure)
    assert not rec["ix"].any() and not rec["iy"].any()
    p_gas = run.records["p"][C.gas(run.records)]
    assert (p_gas > 1.0e3).all() and (p_gas < 1.0e7).all()
    dx, dy = 2.0 * float(rec["x"][0, 0]), 2.0 * float(rec["y"][0, 0])
    assert dx > 0 and dy > 0
    eps = float(np.finfo(rec["x"].dtype).eps)
    np.testing.assert_allclose(rec["x"], (i + 0.5) * dx, rtol=4 * eps)
    np.testing.assert_allclose(rec["y"], (j + 0.5) * dy, rtol=4 * eps)
    assert not (rec["nb_ptr"] != 0).any()
    assert (C.gas(run.records).sum(), (~C.gas(run.records)).sum()) == (796, 55)   # the wedge's solid cells


@pytest.mark.parametrize("deck", C.SEVEN)
def test_both_compilers_builds_write_the_same_records(cpu_fp32, deck):
    """hf2d_fp32 --backend cpu against the g++ build hf2d_cpu_fp32, from the
    same perturbed seed: rule "equal" (on the resonator only the payloads of
    the non-finite k / eps words may differ)."""
    ref = C.cpu_reference(deck)
    run = C.finished(C.march(C.seed_of(deck), cpu_fp32, "cpu"))
    assert run.profile[0]["path"] == {} and ref.profile[0]["path"] == {}   # the CPU solver has one path
    bad = C.equal_misses(run, ref) + C.plt_misses(run, ref)
    assert not bad, "; ".join(bad)
    finite = all(np.isfinite(ref.records[n]).all() for n in C._real_fields(C.REC32))
    assert finite == (deck not in C.NONFINITE_OK)
    if finite:
        assert run.hf2d == ref.hf2d


@pytest.mark.parametrize("deck", ["wedge_37x23", "wedge_keps_48x24", "triple_48x24"])
def test_float_cpu_stepper_on_three_ranks_equals_one(hf, deck):
    ref = C.cpu_reference(deck)
    port = 29700 + ["wedge_37x23", "wedge_keps_48x24", "triple_48x24"].index(deck)
    run = C.finished(C.march(C.seed_of(deck), C.GPU_FP32, "cpu", ranks=3, env={"MASTER_PORT": port}))
    assert "halo transport tcp" in run.stdout
    assert [p["rank"] for p in run.profile] == [0, 1, 2]
    assert run.hf2d == ref.hf2d
    bad = C.plt_misses(run, ref)
    assert not bad, "; ".join(bad)


def test_equal_rule_notices_one_bit_and_one_moved_nan():
    """The rules' own bite: a last-place change of one value, and a non-finite
    value in another cell than the reference's."""
    ref = C.cpu_reference("resonator_37x23")
    assert C.equal_misses(ref, ref) == []
    rec = ref.records.copy()
    rec["U"][5] = np.nextafter(rec["U"][5], np.float32(np.inf))
    moved = ref._replace(records=rec, hf2d=rec.tobytes())
    assert len(C.equal_misses(moved, ref)) == 1 and C.equal_misses(moved, ref)[0].startswith(
        "U: 1 cells differ (first: record 5), 1 by value")
    assert C.distances(moved, ref)[0]["U"] > 0
    rec = ref.records.copy()
    cell = int(np.nonzero(np.isfinite(rec["S"][:, 7]))[0][0])
    rec["S"][cell, 7] = np.nan
    moved = ref._replace(records=rec, hf2d=rec.tobytes())
    assert any(m.startswith("S: non-finite") for m in C.equal_misses(moved, ref))
    assert C.distances(moved, ref)[1] == ["S7"]


def test_precision_scale(hf, cpu_fp32, capsys):
    """D = max |cpu_fp32 - cpu_fp64| / max |cpu_fp64| over gas, per "close"
    deck and field: same deck, same random factors, same schedule, bin/hf2d_cpu
    against bin/hf2d_cpu_fp32.  At least 1e-6 on rho, U, V, p, Tg; the
    committed table (tests/golden/fp32_precision_scale.json, which
    test_gpu_fp32_cells.py reads) holds these values.  HF2D_WRITE_GOLDEN=1
    rewrites the file."""
    table = {}
    for deck in C.CLOSE_DECKS:
        lo = C.finished(C.march(C.seed_of(deck, C.NMAX, cpu_fp32), cpu_fp32, "cpu"))
        hi = C.finished(C.march(C.seed_of(deck, C.NMAX, C.CPU_FP64), C.CPU_FP64, "cpu"))
        assert lo.records.dtype == C.REC32 and hi.records.dtype == C.REC64
        assert np.array_equal(C.gas(lo.records), C.gas(hi.records))
        table[deck] = {f: float("%.3e" % d) for f, d in C.distances(lo, hi)[0].items()}
    with capsys.disabled():
        print("\nD, FP32 against FP64 CPU stepper (relative to the field's max over gas)")
        print("%-8s" % "field" + "".join("%18s" % d for d in C.CLOSE_DECKS))
        for f in C.FIELDS:
            print("%-8s" % f + "".join("%18.3e" % table[d][f] for d in C.CLOSE_DECKS))
    for deck in C.CLOSE_DECKS:
        for f in C.SCALE_FIELDS:
            assert table[deck][f] >= 1e-6, (deck, f, table[deck][f])
    if os.environ.get("HF2D_WRITE_GOLDEN") == "1" or not os.path.exists(C.SCALE_JSON):
        with open(C.SCALE_JSON, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
    kept = C.precision_scale()
    assert sorted(kept) == C.CLOSE_DECKS
    for deck in C.CLOSE_DECKS:
        assert sorted(kept[deck]) == sorted(C.FIELDS)
        for f in C.FIELDS:
            # (host libm's expf / powf may differ in the last place between releases)
            assert abs(kept[deck][f] - table[deck][f]) <= 0.05 * table[deck][f], (deck, f, kept[deck][f], table[deck][f])
