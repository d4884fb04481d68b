"""The device solver's knob table (csrc/hip/device_knobs.hpp): defaults,
environment parsing and bindings, through DeviceSolver.knob_table() and
DeviceSolver.knobs_from_env() -- no GPU needed."""
import os

import pytest

# the defaults of the members as they stood in device_solver.hpp before the
# table (cu_count: the table's, a constructed solver takes the device's)
DEFAULTS = {
    "split_xcd": True, "split_xcd_mech": False, "mech_lazy": True, "chem_kernel": 0, "grad_every": False,
    "lnm_ti": 16, "tile_stagger": -150, "host_tail": True, "dt_read_mode": 1, "tile_skip_same": False,
    "lns_ghost_prologue": True, "fill_occ": -1, "lns_occ": 0, "halo_compact": True, "comm_overlap": True,
    "lnm_overlap": False, "chem_fast": True, "chem_compact": True, "chem_rtc": True, "fused": True, "lean": True,
    "lean_tile": True, "lean_sg": True, "lean_tj": 0, "lean_wgcu": 0, "lean_cpt": 2, "lean_nt": 256, "sgl": True,
    "lean_ns": True, "lean_mech": True, "cu_count": 256, "use_graph": True, "p2p_queue_check": True,
    "lnm_timing": False, "p2p_fuse": False,
    # the reads that were scattered over the sources, now rows
    "fx_skip": 0, "fx_edge_first": 0, "fx_count1": 0, "lnm_trace": False, "autotune_enabled": True,
    "p2p_fuse_wanted": True,
}

ENV = {
    "split_xcd": "HF2D_SPLIT_XCD", "split_xcd_mech": "HF2D_SPLIT_XCD_MECH", "mech_lazy": "HF2D_MECH_LAZY",
    "chem_kernel": "HF2D_CHEM_KERNEL", "grad_every": "HF2D_GRAD_EVERY", "lnm_ti": "HF2D_LNM_TI",
    "tile_stagger": "HF2D_STAGGER", "host_tail": "HF2D_HOST_TAIL", "dt_read_mode": "HF2D_DT_READ",
    "tile_skip_same": "HF2D_SKIP_SAME", "lns_ghost_prologue": "HF2D_GHOST_PROLOGUE", "fx_skip": "HF2D_FX_SKIP",
    "fx_edge_first": "HF2D_FX_EDGE_FIRST", "fx_count1": "HF2D_FX_COUNT1", "lnm_trace": "HF2D_LNM_TRACE",
    "autotune_enabled": "HF2D_AUTOTUNE", "p2p_fuse_wanted": "HF2D_P2P_FUSE",
    # which stepper runs and the tile geometry: a native CLI (the FP32 build has no other face) reaches them
    "fused": "HF2D_FUSED", "lean": "HF2D_LEAN", "lean_tile": "HF2D_LEAN_TILE", "lean_sg": "HF2D_LEAN_SG",
    "sgl": "HF2D_SGL", "lean_ns": "HF2D_LEAN_NS", "use_graph": "HF2D_GRAPH", "lean_tj": "HF2D_LEAN_TJ",
    "lean_cpt": "HF2D_LEAN_CPT", "lean_nt": "HF2D_LEAN_NT", "cu_count": "HF2D_CU_COUNT",
}


@pytest.fixture
def clean_env(monkeypatch):
    for k in [k for k in os.environ if k.startswith("HF2D_")]:
        monkeypatch.delenv(k)
    return monkeypatch


def test_knob_defaults_are_pinned(native, clean_env):
    assert native.DeviceSolver.knobs_from_env() == DEFAULTS
    rows = native.DeviceSolver.knob_table()
    assert [r[0] for r in rows] == list(native.DeviceSolver.knobs_from_env())   # one row per knob, in table order
    assert len({r[0] for r in rows}) == len(rows)
    assert {r[0]: r[2] for r in rows} == DEFAULTS
    assert {r[0]: r[3] for r in rows if r[3] is not None} == ENV
    for name, typ, default, env, graph in rows:
        assert typ in ("bool", "int") and type(default).__name__ == typ, name
        assert type(graph) is bool, name


@pytest.mark.parametrize("name", sorted(ENV))
def test_every_environment_row_parses(native, clean_env, name):
    """A non-default value of the row's variable changes that knob and no other."""
    default = DEFAULTS[name]
    if isinstance(default, bool):
        text, want = ("0", False) if default else ("1", True)
    else:
        text, want = str(default + 3), default + 3
    clean_env.setenv(ENV[name], text)
    assert native.DeviceSolver.knobs_from_env() == dict(DEFAULTS, **{name: want})


def test_bool_knobs_are_set_unless_zero(native, clean_env):
    """One rule for every bool row: set and not "0" (HF2D_P2P_FUSE=2 now fuses,
    as the native bootstrap always read it)."""
    clean_env.setenv("HF2D_P2P_FUSE", "2")
    clean_env.setenv("HF2D_SKIP_SAME", "yes")
    got = native.DeviceSolver.knobs_from_env()
    assert got["p2p_fuse_wanted"] is True and got["tile_skip_same"] is True


def test_every_knob_is_a_solver_attribute(native):
    for name, typ, default, env, graph in native.DeviceSolver.knob_table():
        assert hasattr(native.DeviceSolver, name), name
        if graph:
            assert typ in ("bool", "int"), name
    # the knobs the old hand-written signature list left out are graph rows
    graph = {r[0] for r in native.DeviceSolver.knob_table() if r[4]}
    assert {"tile_stagger", "fill_occ", "lns_occ", "split_xcd", "split_xcd_mech", "mech_lazy", "grad_every",
            "chem_kernel", "chem_fast", "chem_rtc", "chem_compact", "lnm_ti", "lnm_overlap", "comm_overlap",
            "halo_compact", "host_tail", "dt_read_mode", "cu_count", "tile_skip_same",
            "lns_ghost_prologue"} <= graph
