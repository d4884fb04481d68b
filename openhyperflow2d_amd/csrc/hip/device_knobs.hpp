// The device solver's tuning knobs: one row each.  The members of DeviceKnobs
// (a base of DeviceSolver), the environment reads (read_env), the step-graph
// signature (DeviceSolver::mode_signature) and the Python attributes
// (bind/module.cpp) are all expanded from this table.  No HIP dependency.
//
//   X(name, type, default, environment variable or nullptr, graph)
//
// name: the C++ member and the Python attribute.  type: bool or int.  graph: a
// launch issued from do_step_eager (or anything it calls) reads the knob for
// its kernel pointer, grid, LDS size or arguments, so a captured step-graph
// window bakes it in and must not replay after it changed.
// Every setting gives bitwise-identical results unless its row says otherwise.
#pragma once

#include <cstdlib>
#include <cstring>

// clang-format off
#define HF2D_DEVICE_KNOBS(X) \
  /* ---- which stepper runs ---- */ \
  /* Euler: single fused predict+fill kernel */ \
  X(fused, bool, true, "HF2D_FUSED", true) \
  /* inviscid: lean kernel on the reduced state (lean_euler.hpp) when the case is eligible; takes precedence over `fused` */ \
  X(lean, bool, true, "HF2D_LEAN", true) \
  /* LDS-tiled lean kernel for all but the first lean step */ \
  X(lean_tile, bool, true, "HF2D_LEAN_TILE", true) \
  /* single-gas specialisation (lean_euler.hpp) if eligible (lean_sg_ok) */ \
  X(lean_sg, bool, true, "HF2D_LEAN_SG", true) \
  /* single-gas laminar N-S specialisation (stepkern.hpp fill_cell<SGL>) if eligible (sgl_ok) */ \
  X(sgl, bool, true, "HF2D_SGL", true) \
  /* single-gas laminar N-S: one LDS-tiled kernel per step with the fluxes recomputed in the tile (hip/lean_ns.hpp) when eligible (lns_ok) */ \
  X(lean_ns, bool, true, "HF2D_LEAN_NS", true) \
  /* mechanism mode: the lean step of hip/lean_mech.hpp (tile kernel + kinetics + reacting-cell state kernel) when eligible (lnm_ok) */ \
  X(lean_mech, bool, true, nullptr, true) \
  /* step graphs: 6-step windows captured once and replayed (device_solver.hip) */ \
  X(use_graph, bool, true, "HF2D_GRAPH", false) \
  /* ThreadBlockSize = 0 times the lean tile geometries before the first step; 0: skip the search */ \
  X(autotune_enabled, bool, true, "HF2D_AUTOTUNE", false) \
  /* ---- inviscid lean tile kernel ---- */ \
  /* tile height override (0: auto, ny split in <= 64) */ \
  X(lean_tj, int, 0, "HF2D_LEAN_TJ", true) \
  /* >0: at most this many tile workgroups resident per CU (LDS request) */ \
  X(lean_wgcu, int, 0, nullptr, true) \
  /* cells per thread in the tiled kernel: 1 or 2 (2: measured ~20% faster) */ \
  X(lean_cpt, int, 2, "HF2D_LEAN_CPT", true) \
  /* threads per tile workgroup: 256, or 128 / 64 (single gas; small strips) */ \
  X(lean_nt, int, 256, "HF2D_LEAN_NT", true) \
  /* compute units (the constructor overwrites it from the device properties): the cpt gate and the stagger rounds */ \
  X(cu_count, int, 256, "HF2D_CU_COUNT", true) \
  /* staggered start of the tile kernel's resident dispatch rounds, 10 ns ticks per round of cu_count workgroups; > 0 whole */ \
  /* rounds, < 0 a linear ramp (headline 2000x200, 1x MI355X, after the fast divide: off 31.3 us, rounds of 1.5 us 29.9 us; */ \
  /* ramp of 0.5 / 1.0 / 1.5 / 2.0 / 3.0 us per round 30.7 / 30.1 / 29.6 / 30.4 / 32.3 us) */ \
  X(tile_stagger, int, -150, "HF2D_STAGGER", true) \
  /* dt read (StepParams::dt_read / dt_fold): 0 word + shards by scalar loads, 1 by one vector load per lane, 2 the previous */ \
  /* step's last workgroup folds them into the word (single GPU) */ \
  X(dt_read_mode, int, 1, "HF2D_DT_READ", true) \
  /* skip stores of beta / CP whose bits did not change */ \
  X(tile_skip_same, bool, false, "HF2D_SKIP_SAME", true) \
  /* single GPU: the last tile step of a host call writes dt / time / the error flag into the pinned host mirror from its */ \
  /* own tail, instead of a separate read-back kernel after it (0: off) */ \
  X(host_tail, bool, true, "HF2D_HOST_TAIL", true) \
  /* ---- split predict / fill kernels ---- */ \
  /* fill kernels: -1 auto, 0 compiler default, 2/3/4 waves-per-SIMD register budget */ \
  X(fill_occ, int, -1, nullptr, true) \
  /* XCD-aware workgroup order (0: round robin) */ \
  X(split_xcd, bool, true, "HF2D_SPLIT_XCD", true) \
  /* ... also for the mechanism pair (measured 2 % slower) */ \
  X(split_xcd_mech, bool, false, "HF2D_SPLIT_XCD_MECH", true) \
  /* mechanism N-S fill: species gradients/fluxes inside the heat flux (0: stored) */ \
  X(mech_lazy, bool, true, "HF2D_MECH_LAZY", true) \
  /* SGT / mechanism fill: store the gradients every step, not only on outputs */ \
  X(grad_every, bool, false, "HF2D_GRAD_EVERY", true) \
  /* ---- lean N-S / mechanism tile steps ---- */ \
  /* lean N-S kernel: 0 compiler register budget; 5 / 6: waves-per-SIMD budget */ \
  X(lns_occ, int, 0, nullptr, true) \
  /* fused lean N-S steps: the next fused step's edge tiles unpack the last step's halo from the mailbox (0: separate unpack launch) */ \
  X(lns_ghost_prologue, bool, true, "HF2D_GHOST_PROLOGUE", true) \
  /* mechanism tile columns (16 rows): 16 or 12 (lean_mech.hpp lnm_tile) */ \
  X(lnm_ti, int, 16, "HF2D_LNM_TI", true) \
  /* mechanism step: edge tiles first, halo overlapped with the interior (opt-in) */ \
  X(lnm_overlap, bool, false, nullptr, true) \
  /* measurement: per-phase device time of the lean mechanism step in lnm_phase_ms; the host waits for every step's events (eager) */ \
  X(lnm_timing, bool, false, nullptr, false) \
  /* in-kernel phase trace of every lean mechanism step, 12 clocks / ids per workgroup (lnm_trace_fetch); set by the variable being present */ \
  X(lnm_trace, bool, false, "HF2D_LNM_TRACE", true) \
  /* ---- kinetics ---- */ \
  /* 0 auto (compiled VALU kernel if the mechanism has one, else the hiprtc-specialised one, else the MFMA kernel), */ \
  /* 1 compiled, 2 MFMA, 3 generic runtime-data VALU, 4 hiprtc-specialised */ \
  X(chem_kernel, int, 0, "HF2D_CHEM_KERNEL", true) \
  /* compiled-mechanism kinetics kernel when one exists (chem_fast_ok) */ \
  X(chem_fast, bool, true, nullptr, true) \
  /* compiled kinetics over a compacted list of the reacting cells */ \
  X(chem_compact, bool, true, nullptr, true) \
  /* a mechanism without built-in kernels: hiprtc-specialised chem_fast kernels (chem_rtc.hip, compiled at upload, code object */ \
  /* cached) instead of the runtime-data MFMA kernel; kernel kind 4 */ \
  X(chem_rtc, bool, true, nullptr, true) \
  /* ---- halo transport ---- */ \
  /* split-path halos carry only what the next kernels read of a ghost column (halo_fields); false: every field of the group */ \
  X(halo_compact, bool, true, nullptr, true) \
  /* RCCL / in-process transports: halo of the edge tiles on a comm stream while the interior tiles compute, then the dt MIN */ \
  X(comm_overlap, bool, true, nullptr, true) \
  /* fold the p2p exchange into the lean tile kernels (hf2d_lean_tile_fx); set by the bootstrap after validation */ \
  X(p2p_fuse, bool, false, nullptr, true) \
  /* what the bootstrap copies into p2p_fuse once the mailboxes are validated (0: a separate exchange kernel) */ \
  X(p2p_fuse_wanted, bool, true, "HF2D_P2P_FUSE", false) \
  /* p2p_import refuses more in-process ranks than HIP hardware queues allow */ \
  X(p2p_queue_check, bool, true, nullptr, false) \
  /* cost attribution of the fused exchange (FusedX::skip; loopback timing runs only, wrong results): skip parts of it, bit 4 traces the tail */ \
  X(fx_skip, int, 0, "HF2D_FX_SKIP", true) \
  /* inviscid fused tile kernel: edge tile columns dispatched first (FusedX::edge_first) */ \
  X(fx_edge_first, int, 0, "HF2D_FX_EDGE_FIRST", true) \
  /* 1 / 2 forces one / two levels of the fused tail's completion count (FusedX::count1; 0: the caller's) */ \
  X(fx_count1, int, 0, "HF2D_FX_COUNT1", true)
// clang-format on

namespace hf2d {

struct DeviceKnobs {
#define HF2D_KNOB_MEMBER(name, type, def, env, graph) type name = def;
  HF2D_DEVICE_KNOBS(HF2D_KNOB_MEMBER)
#undef HF2D_KNOB_MEMBER

  // One rule per type: a bool is "set and not 0", an int goes through atoi.
  static void parse(bool& v, const char* e) { v = std::strcmp(e, "0") != 0; }
  static void parse(int& v, const char* e) { v = std::atoi(e); }
  static const char* env_value(const char* var) { return var ? std::getenv(var) : nullptr; }
  void read_env() {
#define HF2D_KNOB_ENV(name, type, def, env, graph) \
  if (const char* e = env_value(env)) parse(name, e);
    HF2D_DEVICE_KNOBS(HF2D_KNOB_ENV)
#undef HF2D_KNOB_ENV
    if (std::getenv("HF2D_LNM_TRACE")) lnm_trace = true;   // (presence alone arms the trace)
  }
};

}  // namespace hf2d
