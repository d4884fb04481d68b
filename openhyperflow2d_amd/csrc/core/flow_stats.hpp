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
  double t_off = 0.0;    // device: the clock is DevScalars::time_part - t_off (upload() and a cycle roll restart time_part)
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

// Extension (start_averaging's favre / species options): mass fractions of
// listed mechanism species and Favre (density-weighted) averages.  With w, r
// the tick's values of this sample and rho = row[2]:
//   species, for each listed s in list order, Y_s = rho != 0 ? rhoY_s / rho : 0
//   (the division field("Y:<s>") performs on the post-step partial density):
//     d = Y_s - mY_s;  mY_s := mY_s + r * d;  e = Y_s - mY_s
//     MY_s := MY_s + (w * d) * e
//   Favre, per cell with its own weight sum G:
//     om = w * rho;  G1 = G + om;  q = G1 > 0 ? om / G1 : 0;  G := G1
//     for x in (T, U, V, Y_s...):
//       d = x - f_x;  f_x := f_x + q * d;  e = x - f_x;  F_x := F_x + (om * d) * e
//     CF := CF + (om * d_U) * e_V
// in double, in this order, without contraction.  species_var = MY / W,
// favre_var = F / G and favre_cov_uv = CF / G (0 where G == 0) are formed by
// the reader.  Every plane depends on its own history only, so the species and
// the Favre update of Y_s share one pass over the list.
constexpr int STATS_MAX_SPECIES = 16;
constexpr int STATS_FAVRE_BASE = 3;   // T, U, V; the listed species follow

struct StatsExt {
  int ns = 0;                      // listed species
  int sp[STATS_MAX_SPECIES] = {};  // their mechanism indices
  double* mY = nullptr;   // [ns][N] mass-fraction means
  double* MY = nullptr;   // [ns][N] weighted squared deviations (second moments only)
  double* G = nullptr;    // [N] Favre weight sum
  double* f = nullptr;    // [3 + ns][N] Favre means
  double* F = nullptr;    // [3 + ns][N] Favre squared deviations (second moments only)
  double* CF = nullptr;   // [N] Favre U, V co-moment (second moments only)
};

// The base planes of the accumulator on the device (hip/flow_stats.hpp).
struct FlowStats {
  double* m = nullptr;   // [STATS_VARS][N] means
  double* M = nullptr;   // [STATS_VARS][N] weighted squared deviations (second moments only)
  double* C = nullptr;   // [N] weighted U, V co-moment (second moments only)
  StatsScalars* sc = nullptr;
  long c0 = 0, c1 = 0;   // owned cells [c0, c1) of the strip's N (the ghost columns lie outside)
};

// Planes of N doubles one accumulator holds (base, species, Favre).
inline size_t stats_plane_count(bool second_moments, bool favre, int ns) {
  size_t n = second_moments ? 2 * STATS_VARS + 1 : STATS_VARS;
  n += (size_t)ns * (second_moments ? 2 : 1);
  if (favre) n += 1 + (size_t)(STATS_FAVRE_BASE + ns) * (second_moments ? 2 : 1) + (second_moments ? 1 : 0);
  return n;
}

// The extension's pointers into one block of stats_plane_count planes that
// starts with the base planes.
inline void stats_ext_planes(StatsExt& x, double* base, size_t N, bool second_moments, bool favre) {
  double* p = base + (second_moments ? 2 * STATS_VARS + 1 : STATS_VARS) * N;
  auto take = [&](bool on, size_t n) {
    double* q = on && n ? p : nullptr;
    if (on) p += n * N;
    return q;
  };
  const size_t ns = (size_t)x.ns;
  x.mY = take(true, ns);
  x.MY = take(second_moments, ns);
  x.G = take(favre, 1);
  x.f = take(favre, STATS_FAVRE_BASE + ns);
  x.F = take(favre && second_moments, STATS_FAVRE_BASE + ns);
  x.CF = take(favre && second_moments, 1);
}

// One cell: row as stats_cell; Ys the cell's entry of the species block
// [nsp][N] of post-step partial densities; x's planes are indexed with c.
template <bool MOMENTS, bool FAVRE>
HF_HD inline void stats_cell_x(double w, double r, const real* row, const real* Ys, long N, const StatsExt& x, long c) {
  const double rho = (double)row[2];
  double om = 0.0, q = 0.0, dU = 0.0, eV = 0.0;
  if (FAVRE) {
    om = w * rho;
    const double G1 = x.G[c] + om;
    q = G1 > 0.0 ? om / G1 : 0.0;
    x.G[c] = G1;
#pragma unroll
    for (int k = 0; k < STATS_FAVRE_BASE; k++) {
      const double v = (double)row[k == 0 ? 1 : k + 2];   // T, U, V
      const long o = (long)k * N + c;
      const double f0 = x.f[o];
      const double d = v - f0;
      const double f1 = f0 + q * d;
      x.f[o] = f1;
      if (MOMENTS) {
        const double e = v - f1;
        x.F[o] = x.F[o] + (om * d) * e;
        if (k == 1) dU = d;
        if (k == 2) eV = e;
      }
    }
    if (MOMENTS) x.CF[c] = x.CF[c] + (om * dU) * eV;
  }
  for (int s = 0; s < x.ns; s++) {
    const double Y = rho != 0.0 ? (double)Ys[(long)x.sp[s] * N] / rho : 0.0;
    const long o = (long)s * N + c;
    {
      const double m0 = x.mY[o];
      const double d = Y - m0;
      const double m1 = m0 + r * d;
      x.mY[o] = m1;
      if (MOMENTS) {
        const double e = Y - m1;
        x.MY[o] = x.MY[o] + (w * d) * e;
      }
    }
    if (FAVRE) {
      const long of = o + (long)STATS_FAVRE_BASE * N;
      const double f0 = x.f[of];
      const double d = Y - f0;
      const double f1 = f0 + q * d;
      x.f[of] = f1;
      if (MOMENTS) {
        const double e = Y - f1;
        x.F[of] = x.F[of] + (om * d) * e;
      }
    }
  }
}

}  // namespace hf2d
