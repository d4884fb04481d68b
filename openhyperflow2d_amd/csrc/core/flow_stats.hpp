// Time-averaged flow statistics: the update rule shared by the host stepper
// (CpuSolver::after_step) and the device kernels (hip/flow_stats.hpp).
//
// Per cell and variable x in (p, T, rho, U, V) the running weighted mean m,
// the weighted sum of squared deviations M and, for (U, V), the weighted
// co-moment C follow the incremental update of West (1979), the weighted form
// of Welford's: with the sample's weight w and the weight sum W,
//   W1 = W + w;  r = w / W1;  W := W1
//   d = x - m;  m := m + r * d;  e = x - m
//   M := M + (w * d) * e;  C := C + (w * d_U) * e_V
// evaluated in exactly this order in double (also in the real = float build),
// without contraction, so that both sides and a NumPy transcription agree bit
// for bit.  var = M / W and cov = C / W are formed by the reader.
#pragma once

#include "common.hpp"

namespace hf2d {

constexpr int STATS_VARS = 5;   // p, T, rho, U, V (the probe recorder's row)

// Scalar part, run once per step before any cell is touched.
struct StatsScalars {
  double W = 0.0;        // weight sum: the averaged time span (weight = time) or the sample count
  double t_seen = 0.0;   // clock at the last sample (at arming / reset / upload before the first)
  double t_off = 0.0;    // device: the clock is DevScalars::time_part - t_off (upload() restarts time_part)
  double w = 0.0, r = 0.0;   // this step's weight and w / W
  unsigned long long samples = 0, seen = 0;   // samples taken, steps seen since arming / reset
  int sample = 0;        // this step is a sample (the cell pass reads it)
  int every = 1, step_weight = 0;
};

// One step went by at clock t_now: true when it is a sample (every `every`-th
// step, the first one `every` steps after arming); then w, r and W are updated.
HF_HD inline bool stats_tick(StatsScalars& s, double t_now) {
  s.seen += 1;
  s.sample = s.seen % (unsigned long long)s.every == 0 ? 1 : 0;
  if (!s.sample) return false;
  const double w = s.step_weight ? 1.0 : t_now - s.t_seen;
  s.t_seen = t_now;
  const double W1 = s.W + w;
  s.w = w;
  s.r = W1 > 0.0 ? w / W1 : 0.0;   // (no time has passed yet: the sample carries no weight)
  s.W = W1;
  s.samples += 1;
  return true;
}

// One cell: planes m[STATS_VARS][N], M[STATS_VARS][N], C[N]; the pointers are
// the cell's entries of plane 0.
template <bool MOMENTS>
HF_HD inline void stats_cell(double w, double r, const real* row, double* m, double* M, double* C, long N) {
  double dU = 0.0, eV = 0.0;
#pragma unroll
  for (int v = 0; v < STATS_VARS; v++) {
    const double x = (double)row[v];
    const double m0 = m[v * N];
    const double d = x - m0;
    const double m1 = m0 + r * d;
    m[v * N] = m1;
    if (MOMENTS) {
      const double e = x - m1;
      M[v * N] = M[v * N] + (w * d) * e;
      if (v == 3) dU = d;
      if (v == 4) eV = e;
    }
  }
  if (MOMENTS) C[0] = C[0] + (w * dU) * eV;
}

}  // namespace hf2d
