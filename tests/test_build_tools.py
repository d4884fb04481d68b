"""Build-system and plot-helper coverage (Makefile/.compiler fragments,
viewplt.sh, view_RMS.sh).  The CMake test only configures (the full build is exercised by
_build.py through the other tests)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("cmake") is None or not os.path.isdir("/opt/rocm"), reason="cmake/ROCm missing")
def test_cmake_configures(tmp_path):
    r = subprocess.run(["cmake", "-S", ROOT, "-B", str(tmp_path / "b"), "-G", "Ninja"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    ninja = (tmp_path / "b" / "build.ninja").read_text()
    for tgt in ("_hf2d", "hf2d_cpu", "hf2d"):
        assert f"build {tgt}" in ninja
    assert "--offload-arch=gfx950" in ninja
    # every translation unit of csrc/hip is built (bind/module.cpp calls into each)
    hip = os.path.join(ROOT, "openhyperflow2d_amd", "csrc", "hip")
    units = sorted(f for f in os.listdir(hip) if f.endswith(".hip"))
    assert units
    for u in units:
        assert os.path.join("csrc", "hip", u) in ninja, u


LLVM_TOOLS = [os.path.join("/opt/rocm/lib/llvm/bin", t) for t in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")]


@pytest.mark.skipif(not all(os.path.exists(t) for t in LLVM_TOOLS), reason="LLVM binary tools missing")
def test_every_kernel_is_compiled_in_one_code_object(native):
    """The solver is split by kernel family: the extension holds several gfx950 code
    objects and no kernel name occurs in two (metadata notes only, no GPU)."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as kr
    finally:
        sys.path.pop(0)
    objs = kr.resources_by_object(native.__file__)
    assert len(objs) > 1
    assert all(objs), "a code object without kernels in its notes"
    assert kr.duplicates(objs) == []
    assert len(kr.resources(native.__file__)) == sum(len(o) for o in objs)


def test_readme_knobs_are_the_ones_the_code_reads(native):
    """The README's "Device tuning knobs" paragraph and the code agree: every HF2D_*
    variable named there is read somewhere in the package or in bench.py, and every
    variable of the solver's knob table (DeviceSolver.knob_table()) and every
    getenv("HF2D_...") left in the native sources is named in the README.  Under
    csrc/hip only the table header, chem_rtc.hip (the cache path) and LocalGroup
    (the race probe) read HF2D_* variables themselves."""
    import re

    table_env = {row[3] for row in native.DeviceSolver.knob_table() if row[3]}
    assert len(table_env) > 10, table_env

    readme = open(os.path.join(ROOT, "README.md")).read()
    start = readme.index("Device tuning knobs")
    named = set(re.findall(r"HF2D_[A-Z0-9_]+", readme[start:readme.index("\n\n", start)]))
    assert len(named) > 10, named
    pkg = os.path.join(ROOT, "openhyperflow2d_amd")
    texts = {os.path.join(ROOT, "bench.py"): open(os.path.join(ROOT, "bench.py")).read()}
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".hip", ".inc", ".sh")):
                texts[os.path.join(d, f)] = open(os.path.join(d, f), errors="replace").read()
    reads = set()
    for t in texts.values():
        reads |= set(re.findall(r"""(?:getenv\(|environ\.get\(|environ\[)\s*["'](HF2D_[A-Z0-9_]+)["']""", t))
    assert named - (reads | table_env) == set(), "named in the README, read nowhere"
    csrc = os.path.join(pkg, "csrc") + os.sep
    hip = os.path.join(csrc, "hip") + os.sep
    native_reads = set(table_env)
    stray = {}
    for p, t in texts.items():
        if p.startswith(csrc):
            found = set(re.findall(r'getenv\("(HF2D_[A-Z0-9_]+)"', t))
            native_reads |= found
            if found and p.startswith(hip) and os.path.basename(p) not in ("device_knobs.hpp", "chem_rtc.hip"):
                stray[os.path.relpath(p, ROOT)] = found
    assert stray == {os.path.join("openhyperflow2d_amd", "csrc", "hip", "device_solver.hpp"): {"HF2D_LOCAL_JITTER_US"}}, \
        "a solver knob is read outside the knob table"
    assert table_env - named == set(), "in the knob table, not in the README's knob paragraph"
    everywhere = set(re.findall(r"HF2D_[A-Z0-9_]+", readme))
    assert native_reads - everywhere == set(), "read by the native code, not in the README"


def test_plot_helpers_write_gnuplot_scripts(native, tmp_path):
    deck = os.path.join(ROOT, "tests", "fixtures", "ref", "wedge15_200x40_euler", "deck.dat")
    shutil.copy(deck, tmp_path / "deck.dat")
    cli = os.path.join(ROOT, "openhyperflow2d_amd", "bin", "hf2d_cpu")
    r = subprocess.run([cli, "deck.dat"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plt = tmp_path / "Wedge15_200x40.plt"
    env = dict(os.environ, PATH="/usr/bin:/bin")   # no gnuplot: scripts only
    r = subprocess.run([os.path.join(ROOT, "tools", "viewplt.sh"), str(plt), "Mach"], capture_output=True,
                       text=True, env=env)
    assert r.returncode == 0, r.stderr
    gp = (tmp_path / "Wedge15_200x40.plt.Mach.gp").read_text()
    assert "using 1:2:13" in gp   # Mach is the 13th variable
    rows = (tmp_path / "Wedge15_200x40.plt.Mach.dat").read_text().split("\n\n")
    assert len(rows) == 40 and all(len(b.strip().splitlines()) == 200 for b in rows)
    r = subprocess.run([os.path.join(ROOT, "tools", "view_RMS.sh"), str(tmp_path / "RMS-Wedge15_200x40.plt")],
                       capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "RMS-Wedge15_200x40.plt.gp").read_text().count("with lines") == 9
