// Whole-field time averages on the device (core/flow_stats.hpp holds the
// update rule): after every step, while armed,
//   hf2d_stats_tick    one lane: advances the step counter, decides whether
//                      the step is a sample and runs the rule's scalar part
//                      (w, r, W) from the device clock
//   hf2d_stats_accum   one gas cell per lane: the cell's row (p, T, rho, U, V)
//                      through probe_row<KIND> (probe_history.hpp), i.e. bit for
//                      bit what a download after the step yields, folded into
//                      the double planes m, M, C
//   hf2d_stats_accum_x the same pass when Favre averages or species statistics
//                      are armed: the base planes, then stats_cell_x's
// Both run on the solver's stream after the step's last kernel, so they are
// captured into the step graphs.  The tick is a kernel of its own, not the tail
// of the cell pass: w and r are then the product of an earlier launch which
// every workgroup reads with plain loads, the update of W races with nobody,
// and there is neither a completion counter nor a second pass over 35 - 211 MB
// of planes behind it.  The step kernels and their argument blocks are
// untouched.
#pragma once

#include "../core/flow_stats.hpp"
#include "probe_history.hpp"

namespace hf2d {

constexpr int STATS_BLOCK = 256;
static_assert(STATS_VARS == PROBE_VARS, "the accumulated row is the probe recorder's");

#ifdef __HIPCC__
__global__ __launch_bounds__(64) void hf2d_stats_tick(StatsScalars* s, const DevScalars* sc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  StatsScalars t = *s;
  (void)stats_tick(t, sc->time_part - t.t_off);
  *s = t;
}

// arming / reset_averaging: an empty accumulation that starts at the clock's
// present value (the planes are cleared by the caller)
__global__ __launch_bounds__(64) void hf2d_stats_rebase(StatsScalars* s, const DevScalars* sc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  s->W = 0.0;
  s->w = s->r = 0.0;
  s->samples = s->seen = 0;
  s->sample = 0;
  s->t_seen = sc->time_part - s->t_off;
}

template <int KIND, bool MOMENTS>
__global__ __launch_bounds__(STATS_BLOCK) void hf2d_stats_accum(StepParams P, SoA s, FlowStats f) {
  if (!f.sc->sample) return;
  const long idx = f.c0 + (long)blockIdx.x * STATS_BLOCK + (long)threadIdx.x;
  if (idx >= f.c1) return;
  // (before probe_row: a solid node must not enter the lean N-S fill)
  const u64 ct = s.CT[idx];
  if (has_all(ct, CT_SOLID) || !has_all(ct, CT_NODE_IS_SET)) return;
  real row[PROBE_VARS];
  probe_row<KIND>(P, s, idx, row);
  stats_cell<MOMENTS>(f.sc->w, f.sc->r, row, f.m + idx, f.M + idx, f.C + idx, s.N);
}

// The cell pass with the favre / species options armed (stats_cell_x), in
// place of hf2d_stats_accum: the same lane-per-cell layout and the same row,
// evaluated once, then the base planes and the extension's.  The listed
// species' post-step partial densities are s.Ys (post_step_view); their
// indices and the plane pointers travel in x, so the species loop's trip count
// and plane offsets are wave-uniform.  Every plane is read and written once
// per sample, consecutive lanes on consecutive doubles: 16 B per plane and
// cell-sample, HBM-bound like the base pass.
static_assert(sizeof(StepParams) + sizeof(SoA) + sizeof(FlowStats) + sizeof(StatsExt) + 32 <= 4096,
              "kernel-argument segment");
template <int KIND, bool MOMENTS, bool FAVRE>
__global__ __launch_bounds__(STATS_BLOCK) void hf2d_stats_accum_x(StepParams P, SoA s, FlowStats f, StatsExt x) {
  if (!f.sc->sample) return;
  const long idx = f.c0 + (long)blockIdx.x * STATS_BLOCK + (long)threadIdx.x;
  if (idx >= f.c1) return;
  const u64 ct = s.CT[idx];
  if (has_all(ct, CT_SOLID) || !has_all(ct, CT_NODE_IS_SET)) return;
  real row[PROBE_VARS];
  probe_row<KIND>(P, s, idx, row);
  const double w = f.sc->w, r = f.sc->r;
  stats_cell<MOMENTS>(w, r, row, f.m + idx, f.M + idx, f.C + idx, s.N);
  stats_cell_x<MOMENTS, FAVRE>(w, r, row, s.Ys + idx, s.N, x, idx);
}
#endif

}  // namespace hf2d
