"""The FP32 GPU build cell for cell against the FP32 CPU stepper: record
layout, seeding, marching, comparison rules and the row table (a plain module,
no fixtures; its own evidence on the CPU: test_fp32_cases.py, the GPU rows:
test_gpu_fp32_cells.py).

bin/hf2d_fp32 is the native CLI with every device kernel compiled for
real = float; `--backend cpu` runs the float build of the plain per-cell CPU
stepper from the same binary, and that is the reference of every row: both
sides evaluate the same float expressions, so the distance between them is
not the FP32 / FP64 gap that test_gpu_fp32.py's tolerance has to admit.

Protocol.  seed() runs the deck (Nmax 12, NOutStep 6; graph rows Nmax 30) one
cycle on the CPU backend and perturbs the checkpoint as tests/perturb.py does
with amp 0.02 (every cell then differs from its neighbours); march() restarts
a copy of that directory through bin/OpenHyperFLOW2D.sh for `--cycles 2` with
HF2D_AUTOTUNE=0 and --profile, so the cycle boundary and the y+ kernels run,
and returns the records, the Tecplot files and the profile, whose "path"
object says which kernels ran.

Comparison rules (gas = every record without CT_SOLID):

  "equal"  the .hf2d files are byte-equal; where the CPU file holds
           non-finite floats (the resonator's k / eps in cells nothing is
           transported into) the non-finite values sit in the same words and
           every other word is bit-equal.  Inviscid rows: both sides evaluate
           the same float expressions, the device build has -ffp-contract=off,
           the x86 host contracts nothing, hf_div / hf_sqrt promote to the
           same correctly rounded double operation.
  "close"  per field of FIELDS, max |gpu - cpu| over gas <= bound * max |cpu|
           over gas, and equal non-finite masks.  bound = 4 x the difference
           recorded on an MI355X (MEASURED; the run is deterministic, the
           margin is for a last-place change of device expf / powf / tanhf
           between ROCm releases), subject to bound <= D / 4 with D the
           distance between the FP32 and the FP64 CPU stepper on the same
           deck, start and schedule (tests/golden/fp32_precision_scale.json,
           written and checked by test_fp32_cases.py): a float kernel no
           closer to the float CPU stepper than a quarter of the distance
           between the precisions is not doing the same arithmetic.
  "equal values"  what a measured row is held to when every named field
           recorded 0 (all seven did): every record field bit-equal, +0 and -0
           taken as equal, less the exceptions of UNNAMED; why the files
           cannot be byte-equal is written beside MEASURED."""
import atexit
import collections
import functools
import json
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "openhyperflow2d_amd", "bin")
LAUNCHER = os.path.join(BIN, "OpenHyperFLOW2D.sh")
GPU_FP32 = os.path.join(BIN, "hf2d_fp32")        # device kernels in float; --backend cpu: the reference
CPU_FP32 = os.path.join(BIN, "hf2d_cpu_fp32")    # the g++ build of the same host code (_build.build_fp32)
CPU_FP64 = os.path.join(BIN, "hf2d_cpu")
SCALE_JSON = os.path.join(ROOT, "tests", "golden", "fp32_precision_scale.json")

NEQ, NSPEC = 9, 4
CT_SOLID = 0x040000000
SEED, AMP = 1, 0.02
NMAX, NOUT, NMAX_GRAPH = 12, 6, 30
CYCLES = 2
LIMIT = 120            # seconds, every subprocess
FAULT_STATUS = (124, 137, 134, 139)
FAULT_TEXT = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure",
              "Segmentation fault", "Aborted")


def record_dtype(real):
    """CellRecord of core/common.hpp, fields in struct order, C alignment."""
    r, i4, u8 = np.dtype(real), np.int32, np.uint64
    return np.dtype([
        ("S", r, NEQ), ("dSdx", r, NEQ), ("dSdy", r, NEQ),
        ("TurbType", u8), ("l_min", r), ("y_plus", r), ("Re_local", r), ("mu_t", r), ("lam_t", r),
        ("dkdx", r), ("dkdy", r), ("depsdx", r), ("depsdy", r),
        ("x", r), ("y", r), ("ix", i4), ("iy", i4), ("nb_ptr", u8, 4), ("p", r),
        ("idXl", i4), ("idYu", i4), ("idXr", i4), ("idYd", i4), ("NGX", i4), ("NGY", i4), ("CT", u8),
        ("i_wall", i4), ("j_wall", i4), ("beta", r, NEQ), ("Q_conv", r), ("time", r),
        ("k", r), ("R", r), ("lam", r), ("mu", r), ("CP", r), ("Diff", r), ("Tf", r),
        ("A", r, NEQ), ("B", r, NEQ), ("F", r, NEQ), ("RX", r, NEQ), ("RY", r, NEQ), ("Src", r, NEQ),
        ("SrcAdd", r, NEQ), ("Tg", r), ("U", r), ("V", r), ("Y", r, NSPEC), ("Uw", r), ("Vw", r),
        ("droYdx", r, NSPEC), ("droYdy", r, NSPEC),
        ("dUdx", r), ("dUdy", r), ("dVdx", r), ("dVdy", r), ("dTdx", r), ("dTdy", r), ("BGX", r), ("BGY", r),
    ], align=True)


REC32, REC64 = record_dtype(np.float32), record_dtype(np.float64)
assert REC32.itemsize == 680 and REC64.itemsize == 1248, (REC32.itemsize, REC64.itemsize)

# the fields the "close" rule names: S0..S8 one by one, Y over its four slots
FIELDS = ["S%d" % q for q in range(NEQ)] + ["p", "Tg", "U", "V", "Y", "k", "R", "lam", "mu", "CP", "Diff", "mu_t",
                                            "lam_t", "y_plus"]
SCALE_FIELDS = ["S0", "U", "V", "p", "Tg"]      # rho, U, V, p, Tg: D must be a usable scale (>= 1e-6)


def field(rec, name):
    """Field `name` of FIELDS from a record array, as float64."""
    if name[0] == "S" and name[1:].isdigit():
        return rec["S"][:, int(name[1:])].astype(np.float64)
    return rec[name].astype(np.float64)


def gas(rec):
    return (rec["CT"] & np.uint64(CT_SOLID)) == 0


def grid_of(text):
    return tuple(int(re.search(r"<data/%s=\s*(\d+)" % k, text).group(1)) for k in ("MaxX", "MaxY"))


def flat_fraction(rec, nx, ny):
    """Fraction of the gas cells whose rho, U, V, p equal, bit for bit, those
    of all their (up to four) neighbours inside the grid (tests/perturb.py's,
    on records; x-major: record i * ny + j)."""
    word = np.uint32 if rec.dtype.itemsize == 680 else np.uint64
    flat = np.ones((nx, ny), dtype=bool)
    for a in (rec["S"][:, 0], rec["U"], rec["V"], rec["p"]):
        a = np.ascontiguousarray(a).view(word).reshape(nx, ny)
        same = np.ones(a.shape, dtype=bool)
        same[1:, :] &= a[1:, :] == a[:-1, :]
        same[:-1, :] &= a[:-1, :] == a[1:, :]
        same[:, 1:] &= a[:, 1:] == a[:, :-1]
        same[:, :-1] &= a[:, :-1] == a[:, 1:]
        flat &= same
    g = gas(rec).reshape(nx, ny)
    return float(flat[g].sum()) / max(int(g.sum()), 1)


# ---------------------------------------------------------------------------
# decks
# ---------------------------------------------------------------------------
def _nout(nmax):
    """NOutStep 6 at Nmax 12.  A step graph is a window of six steps without
    an output step, begun at a multiple of six: with an output every sixth
    step none is ever captured, so the graph decks (Nmax 30) take their only
    output step at the head of each cycle and replay steps 6..29."""
    return NOUT if nmax == NMAX else nmax


def _decks():
    from openhyperflow2d_amd.models import decks

    def plate(nmax):
        return decks.set_key(decks.flat_plate(37, 23, turbulence=6, nmax=nmax, nout=_nout(nmax)), "isAdiabaticWall", 1)

    def wedge(nx, ny, **kw):
        return lambda nmax: decks.wedge15(nx, ny, nmax=nmax, nout=_nout(nmax), **kw)

    return {
        "wedge_37x23": wedge(37, 23),
        "wedge_37x33": wedge(37, 33),
        "wedge_221x41": wedge(221, 41),
        "wedge_40x7": wedge(40, 7),
        "wedge_laminar_48x24": wedge(48, 24, navier_stokes=True, turbulence=0),
        "wedge_keps_48x24": wedge(48, 24, navier_stokes=True, turbulence=4),
        "triple_48x24": lambda nmax: decks.triple_point(48, 24, nmax=nmax, nout=NOUT),
        "triple_160x51": lambda nmax: decks.triple_point(160, 51, nmax=nmax, nout=NOUT),
        "step_37x23": lambda nmax: decks.step(37, 23, nmax=nmax, nout=_nout(nmax)),
        "resonator_37x23": lambda nmax: decks.resonator(37, 23, nmax=nmax, nout=NOUT),
        "plate_sst_37x23": plate,
        # strips through the mailboxes (test_gpu_fp32_cells.py, section C)
        "wedge_96x24": wedge(96, 24),
        "wedge_96x24_lagged": lambda nmax: decks.set_key(decks.wedge15(96, 24, nmax=nmax, nout=NOUT), "LaggedDt", 1),
        "resonator_96x24": lambda nmax: decks.resonator(96, 24, nmax=nmax, nout=NOUT),
        "triple_96x24": lambda nmax: decks.triple_point(96, 24, nmax=nmax, nout=NOUT),
        "wedge_keps_96x24": wedge(96, 24, navier_stokes=True, turbulence=4),
    }


# one deck of every family the rows use: what test_fp32_cases.py runs on both compilers' builds
SEVEN = ["wedge_37x23", "wedge_laminar_48x24", "wedge_keps_48x24", "triple_48x24", "step_37x23", "resonator_37x23",
         "plate_sst_37x23"]
# decks whose reference leaves non-finite values on gas cells, and the fields that carry them
NONFINITE_OK = {"resonator_37x23": ("S7", "S8"), "resonator_96x24": ("S7", "S8")}


@functools.lru_cache(maxsize=None)
def deck_text(deck, nmax=NMAX):
    return _decks()[deck](nmax)


# ---------------------------------------------------------------------------
# seeding and marching
# ---------------------------------------------------------------------------
_TMP = []


def _tmpdir():
    d = tempfile.mkdtemp(prefix="hf2d_fp32_")
    _TMP.append(d)
    return d


@atexit.register
def _cleanup():
    for d in _TMP:
        shutil.rmtree(d, ignore_errors=True)


def _records(path, nx, ny):
    size = os.path.getsize(path)
    dt = {nx * ny * 680: REC32, nx * ny * 1248: REC64}[size]
    return np.fromfile(path, dtype=dt)


def _hf2d(d):
    names = [n for n in os.listdir(d) if n.endswith(".hf2d")]
    assert len(names) == 1, names
    return os.path.join(d, names[0])


def perturb_records(rec):
    """tests/perturb.py's perturb() on a record array, in place: S[0:4] of
    every cell times 1 + AMP * r1, S[1:3] times a further 1 + 0.4 * AMP * r2
    (formed in double, stored in the record's precision)."""
    rng = np.random.default_rng(SEED)
    r = rng.uniform(-1.0, 1.0, size=(rec.shape[0], 2))
    S = rec["S"][:, :4].astype(np.float64)
    S *= (1.0 + AMP * r[:, 0])[:, None]
    S[:, 1:3] *= (1.0 + 0.4 * AMP * r[:, 1])[:, None]
    rec["S"][:, :4] = S.astype(rec["S"].dtype)


def seed(text, exe):
    """A directory holding the deck (D.dat), the checkpoint of one CPU cycle
    of `exe` perturbed by perturb_records, and the checkpoint's sidecars."""
    d = _tmpdir()
    with open(os.path.join(d, "D.dat"), "w") as f:
        f.write(text)
    r = subprocess.run(["timeout", "-k", "10", str(LIMIT), exe, "--backend", "cpu", "--cycles", "1", "D.dat"], cwd=d,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "Computation finished" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    nx, ny = grid_of(text)
    path = _hf2d(d)
    rec = _records(path, nx, ny)
    perturb_records(rec)
    rec.tofile(path)
    for n in os.listdir(d):
        if n.endswith(".plt"):
            os.remove(os.path.join(d, n))
    return d


@functools.lru_cache(maxsize=None)
def seed_of(deck, nmax=NMAX, exe=GPU_FP32):
    """seed() of a deck of the table, once per session."""
    return seed(deck_text(deck, nmax), exe)


Run = collections.namedtuple("Run", "returncode stdout stderr records hf2d plt profile grid")


def march(dir, exe, backend="cpu", ranks=1, env=None, cycles=CYCLES):
    """Restart a copy of the seed directory `dir` with `exe` on `ranks` ranks.
    env: {name without the HF2D_ prefix: value}.  Returns Run: the records,
    the .hf2d bytes, {name: bytes} of every .plt, the parsed profile of every
    rank (a list), or None for what a failed run did not write."""
    d = _tmpdir()
    for n in os.listdir(dir):
        if not n.endswith(".plt"):
            shutil.copy(os.path.join(dir, n), os.path.join(d, n))
    e = dict(os.environ, HF2D_BIN=exe, HF2D_AUTOTUNE="0")
    for k, v in (env or {}).items():
        e["HF2D_" + k] = str(v)
    cmd = ["timeout", "-k", "10", str(LIMIT), LAUNCHER, "D", str(ranks), "--backend", backend, "--cycles", str(cycles),
           "--profile", "profile.json"]
    r = subprocess.run(cmd, cwd=d, capture_output=True, text=True, env=e)
    with open(os.path.join(d, "D.dat")) as f:
        nx, ny = grid_of(f.read())
    rec = raw = plt = prof = None
    if r.returncode == 0:
        path = _hf2d(d)
        rec = _records(path, nx, ny)
        rec.setflags(write=False)
        with open(path, "rb") as f:
            raw = f.read()
        plt = {}
        for n in sorted(os.listdir(d)):
            if n.endswith(".plt"):
                with open(os.path.join(d, n), "rb") as f:
                    plt[n] = f.read()
        prof = []
        for q in range(ranks):
            with open(os.path.join(d, "profile.json" + (".rank%d" % q if ranks > 1 else ""))) as f:
                prof.append(json.load(f))
    shutil.rmtree(d, ignore_errors=True)
    return Run(r.returncode, r.stdout, r.stderr, rec, raw, plt, prof, (nx, ny))


def faulted(run):
    """The run ended in a time limit, an abort, a segmentation fault or a HIP
    fault message: nothing more may start on the GPU after it."""
    text = run.stdout[-20000:] + run.stderr[-20000:]
    return run.returncode in FAULT_STATUS or any(t in text for t in FAULT_TEXT)


def finished(run):
    assert run.returncode == 0 and "Computation finished" in run.stdout, \
        "exit %d\n%s\n%s" % (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
    return run


# ---------------------------------------------------------------------------
# the CPU reference of a (deck, nmax): hf2d_fp32 --backend cpu, one rank
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cpu_reference(deck, nmax=NMAX):
    d = seed_of(deck, nmax)
    nx, ny = grid_of(deck_text(deck, nmax))
    start = _records(_hf2d(d), nx, ny)
    assert start.dtype == REC32
    assert flat_fraction(start, nx, ny) == 0.0
    run = finished(march(d, GPU_FP32, "cpu"))
    assert "preloaded" in run.stdout, run.stdout[-2000:]
    g = gas(run.records)
    for f in FIELDS:
        a = field(run.records, f)[g]
        if f in NONFINITE_OK.get(deck, ()):
            assert np.isfinite(a).any(), f
        else:
            assert np.isfinite(a).all(), "%s: %d non-finite gas values" % (f, int((~np.isfinite(a)).sum()))
    assert flat_fraction(run.records, nx, ny) <= 0.02
    return run


# ---------------------------------------------------------------------------
# comparison rules
# ---------------------------------------------------------------------------
def _real_fields(dt):
    return [n for n in dt.names if dt[n].base.kind == "f"]


def equal_misses(run, ref, zero_signs=True, skip=()):
    """Rule "equal" on the .hf2d bytes; returns one line per miss.
    zero_signs=False: +0 and -0 count as equal (rule "equal values");
    skip: record fields left out."""
    if run.hf2d == ref.hf2d:
        return []
    a, b = run.records, ref.records
    if a.dtype != b.dtype or a.shape != b.shape:
        return ["record files of different layouts"]
    word = np.uint32 if a.dtype == REC32 else np.uint64
    bad = []
    for n in a.dtype.names:
        if n in skip:
            continue
        x, y = np.ascontiguousarray(a[n]), np.ascontiguousarray(b[n])
        if n in _real_fields(a.dtype):
            nf = ~np.isfinite(y)
            if not np.array_equal(~np.isfinite(x), nf):
                bad.append("%s: non-finite values in other cells than the reference's" % n)
                continue
            differ = (x.view(word) != y.view(word)) & ~nf
            if not zero_signs:
                differ &= x != y
        else:
            differ = x != y
        if differ.any():
            cells = np.unique(np.nonzero(differ)[0])
            text = "%s: %d cells differ (first: record %d)" % (n, cells.size, int(cells[0]))
            if n in _real_fields(a.dtype):   # how many of them by value, not only in the sign of a zero
                by_value = differ & (x != y)
                text += ", %d by value" % np.unique(np.nonzero(by_value)[0]).size
                if by_value.any():
                    q = tuple(v[0] for v in np.nonzero(by_value))
                    text += " (first: %s %r against %r)" % (q, float(x[q]), float(y[q]))
            bad.append(text)
    if zero_signs and not skip and not bad and not any((~np.isfinite(b[n])).any() for n in _real_fields(b.dtype)):
        bad.append("files differ outside the records' named fields")
    return bad


def _rms_rows(blob):
    return np.array([[float(v) for v in line.split()] for line in blob.decode().splitlines()
                     if line and not line.startswith("#")])


def plt_misses(run, ref):
    """Every Tecplot file byte-equal.  Between runs on different numbers of
    ranks the residual history RMS-<Project>.plt is compared by value instead:
    its entries are sums over the cells accumulated in `real`, every rank
    sums its own strip first, and a float sum of n terms in another order
    differs by up to n * eps relative (plus half a unit of the six printed
    digits); the maxima and the step numbers are order-free."""
    if sorted(run.plt) != sorted(ref.plt):
        return ["other .plt files: %s against %s" % (sorted(run.plt), sorted(ref.plt))]
    bad = []
    for n in sorted(ref.plt):
        if run.plt[n] == ref.plt[n]:
            continue
        if n.startswith("RMS-") and len(run.profile) != len(ref.profile):
            a, b = _rms_rows(run.plt[n]), _rms_rows(ref.plt[n])
            tol = ref.grid[0] * ref.grid[1] * float(np.finfo(np.float32).eps) + 1.0e-5
            if a.shape == b.shape and np.array_equal(a[:, 0], b[:, 0]) and np.allclose(a, b, rtol=tol, atol=0.0):
                continue
        bad.append("%s differs" % n)
    return bad


def distances(run, ref):
    """{field: max |run - ref| over gas / max |ref| over gas} over the cells
    finite in the reference, and the fields whose non-finite masks differ."""
    g = gas(ref.records)
    out, masks = {}, []
    for f in FIELDS:
        x, y = field(run.records, f)[g], field(ref.records, f)[g]
        fin = np.isfinite(y)
        if not np.array_equal(np.isfinite(x), fin):
            masks.append(f)
        fin &= np.isfinite(x)
        top = float(np.abs(y[fin]).max()) if fin.any() else 0.0
        d = float(np.abs(x[fin] - y[fin]).max()) if fin.any() else 0.0
        out[f] = d / top if top > 0 else d
    return out, masks


def record_distance(run, ref, name):
    """max |run - ref| / max |ref| of one record field over the gas cells."""
    g = gas(ref.records)
    x, y = run.records[name][g].astype(np.float64), ref.records[name][g].astype(np.float64)
    top = float(np.abs(y).max())
    d = float(np.abs(x - y).max())
    return d / top if top > 0 else d


def precision_scale():
    with open(SCALE_JSON) as f:
        return json.load(f)


# ---------------------------------------------------------------------------
# the rows of section A (test_gpu_fp32_cells.py): GPU FP32 against CPU FP32
# ---------------------------------------------------------------------------
Row = collections.namedtuple("Row", "id deck nmax env facts rule")


def _tile(p):
    return p["lean_tile_last"]


def _tiles(p):
    return _tile(p)["nbi"] * _tile(p)["nbj"]


# facts: (what must have run, predicate on the profile's "path" object and the grid)
ROWS = [
    Row("tile_default", "wedge_37x23", NMAX, {"LEAN_TJ": 16},
        [("a tile step, two or more tile columns, ragged in both directions",
          lambda p, g: _tile(p)["nt"] != 0 and _tile(p)["nbi"] >= 2 and g[0] % _tile(p)["TI"] != 0
          and g[1] % _tile(p)["TJ"] != 0)], "equal"),
    Row("tile_64x1", "wedge_37x23", NMAX, {"LEAN_NT": 64, "LEAN_CPT": 1, "CU_COUNT": 0},
        [("64 threads, one cell each", lambda p, g: _tile(p)["nt"] == 64 and _tile(p)["cpt"] == 1)], "equal"),
    Row("tile_128x2_tj16", "wedge_37x33", NMAX, {"LEAN_NT": 128, "LEAN_CPT": 2, "LEAN_TJ": 16, "CU_COUNT": 0},
        [("128 threads, two cells each", lambda p, g: _tile(p)["nt"] == 128 and _tile(p)["cpt"] == 2),
         ("three tile rows, the last of one cell",
          lambda p, g: _tile(p)["TJ"] == 16 and _tile(p)["nbj"] == 3 and g[1] - 2 * _tile(p)["TJ"] == 1)], "equal"),
    Row("headline_two_cell", "wedge_221x41", NMAX, {"CU_COUNT": 8, "LEAN_NT": 256, "LEAN_CPT": 2},
        [("256 threads, two cells each", lambda p, g: _tile(p)["nt"] == 256 and _tile(p)["cpt"] == 2),
         ("16 to 32 tiles", lambda p, g: 16 <= _tiles(p) <= 32)], "equal"),
    Row("headline_two_cell_graphs", "wedge_221x41", NMAX_GRAPH,
        {"CU_COUNT": 8, "LEAN_NT": 256, "LEAN_CPT": 2, "GRAPH": 1},
        [("two cells each", lambda p, g: _tile(p)["cpt"] == 2),
         ("step graphs replayed", lambda p, g: p["graph_launches"] > 1)], "equal"),
    Row("three_gas_tile", "triple_48x24", NMAX, {},
        [("the mixture tile kernel", lambda p, g: p["lean_sg_ok"] is False and _tile(p)["nt"] != 0)], "equal"),
    Row("three_gas_two_cell", "triple_160x51", NMAX, {"CU_COUNT": 8},
        [("the mixture tile kernel, two cells each",
          lambda p, g: p["lean_sg_ok"] is False and _tile(p)["cpt"] == 2)], "equal"),
    Row("flat_lean", "wedge_40x7", NMAX, {},
        [("the flat lean kernel", lambda p, g: p["lean_ok"] is True and _tile(p)["nt"] == 0 and _tile(p)["seen"] == 0)],
        "equal"),
    Row("fused_euler", "wedge_37x23", NMAX, {"LEAN": 0},
        [("no lean kernel", lambda p, g: _tile(p)["nt"] == 0 and p["lns_steps"] == 0)], "equal"),
    Row("split_generic", "wedge_37x23", NMAX, {"LEAN": 0, "FUSED": 0},
        [("no lean kernel", lambda p, g: _tile(p)["nt"] == 0 and p["lns_steps"] == 0)], "equal"),
    Row("laminar_lean_ns", "step_37x23", NMAX, {},
        [("the lean N-S tiles", lambda p, g: p["lns_ok"] is True and p["lns_steps"] > 0)], "measured"),
    Row("laminar_split_sgl", "step_37x23", NMAX, {"LEAN_NS": 0},
        [("split SK_SGL", lambda p, g: p["sk_mode"] == 1 and p["split_mode"] == 1 and p["lns_steps"] == 0)], "measured"),
    Row("laminar_generic", "step_37x23", NMAX, {"LEAN_NS": 0, "SGL": 0},
        [("split SK_GENERIC", lambda p, g: p["split_mode"] == 0 and p["lns_steps"] == 0)], "measured"),
    Row("keps_lean_ns_axisym", "resonator_37x23", NMAX, {},
        [("the k-eps lean N-S tiles", lambda p, g: p["lns_turb"] == 2 and p["lns_steps"] > 0)], "measured"),
    Row("keps_split_sgt", "resonator_37x23", NMAX, {"LEAN_NS": 0},
        [("split SK_SGT", lambda p, g: p["sk_mode"] == 2 and p["split_mode"] == 2 and p["lns_steps"] == 0)], "measured"),
    Row("sst_lean_ns", "plate_sst_37x23", NMAX, {},
        [("the SST lean N-S tiles", lambda p, g: p["lns_turb"] == 3 and p["lns_steps"] > 0)], "measured"),
    Row("keps_wall_heat", "wedge_keps_48x24", NMAX, {},
        [("refused by the lean N-S tiles, split SK_SGT",
          lambda p, g: p["lns_ok"] is False and "wall heat transfer" in p["lns_why"] and p["sk_mode"] == 2
          and p["lns_steps"] == 0)], "measured"),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
CLOSE_DECKS = sorted({r.deck for r in ROWS if r.rule == "measured"})

# "measured" rows: {row: {field: largest difference against the CPU reference,
# relative to the field's max over gas, recorded on an MI355X}}.  A row whose
# every field is 0 is held to "equal"; the others to "close" with bound = 4 x
# the value.  A row without an entry fails: it has to be measured first.
#
# Recorded on an MI355X: every field of every row is 0 -- the float
# kernels reproduce the float CPU stepper bit for bit on the viscous paths
# too, device expf / powf / tanhf included, so all seven rows are held to
# "equal" and no bound has to be weighed against D / 4.  (Before
# SolverBase::make_params formed dt / dx from the kernels' float spacings the
# same rows measured up to 5e-7, S2 / V of step_37x23, and the inviscid rows
# were not equal: the host divided by Config's double 0.001, the device by
# 0.001f.)
#
# Held to "equal" these rows still cannot be byte-equal, for two reasons
# found by reading, neither of them in a field the next step reads from a
# neighbour or in the state:
#   - zero signs.  The single-gas specialisations (SK_SGL, SK_SGT, the lean
#     N-S tiles) do not form the fluxes of the frozen species equations and
#     leave +0 in their A / B / F / dSdy slots, where the generic fill stores
#     0 * V = -0 in cells with V < 0 (physics.hpp, n.B[i] = n.S[i] * n.V).
#     Every such word differs in its sign bit only (115 to 357 cells per row,
#     0 by value), and laminar_generic, which runs the generic fill, is
#     byte-equal.  These rows are held to "equal values": every record field
#     bit-equal, +0 and -0 taken as equal.
#   - sst_lean_ns, Src: the omega source of the last fill differs in 2 cells
#     (358596.22 against 358596.38).  It is formed from F1 = tanh(arg1^4)
#     (physics.hpp), and device tanhf differs from the host's in the last
#     place; the run ends before a step reads it.  Src is held to 4 x the
#     recorded distance (UNNAMED), relative to the field's max over gas.
UNNAMED = {"sst_lean_ns": {"Src": 1.047e-11}}   # (max |Src| is 1.5e10, at the wall; 4.4e-7 of the two cells' own value)
MEASURED = {row: dict.fromkeys(FIELDS, 0.0) for row in (
    "laminar_lean_ns", "laminar_split_sgl", "laminar_generic", "keps_lean_ns_axisym", "keps_split_sgt", "sst_lean_ns",
    "keps_wall_heat")}


def rule_of(row):
    if row.rule != "measured":
        return row.rule
    m = MEASURED.get(row.id)
    if m is None:
        return "unmeasured"
    return "equal values" if not any(m.values()) else "close"


def facts_missed(row, run):
    """The row's path facts against every rank's profile; one line per miss."""
    bad = []
    for q, prof in enumerate(run.profile):
        p = prof["path"]
        if p.get("fp") != 32:
            bad.append("rank %d: not the FP32 device solver: %r" % (q, p))
            continue
        for what, pred in row.facts:
            if not pred(p, run.grid):
                bad.append("rank %d: did not run %s: %r" % (q, what, p))
    return bad
