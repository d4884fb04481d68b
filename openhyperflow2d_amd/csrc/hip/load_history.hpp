// Per-step load recorder on the device (core/load_plan.hpp): the pressure and
// friction folds of the body force of every armed box and the mass flow
// through every armed x cut, after every step, bit for bit what x_force_terms /
// y_force_terms / mass_flow_rate_x give on a field downloaded after that step.
//
// Two launches follow the step on the solver's stream, beside the probe
// recorder's, so they are captured into the step graphs:
//   hf2d_loads_terms<KIND>  one lane per term of the plan: the term's value into
//                           a scratch array at the term's position
//   hf2d_loads_fold         one workgroup, one wavefront per list: the list's
//                           scratch slice added in list order into one running
//                           sum (fold_terms' `s = 0; s += t`), then the step's
//                           time and the ring count
// A term reads what a download after the step would hold (KIND: the PR_* kind
// of DeviceSolver::post_step_view):
//   PR_GATHER  generic record, or the lean inviscid arrays (also PR_LEAN): p,
//              mu, mu_t, the gradient slots, U, V and S are stored per cell
//              (the lean inviscid step leaves mu, mu_t and the gradients of the
//              generic arrays alone, and so does its materialise)
//   PR_SGL /   lean N-S state: p, mu, mu_t and the gradient of a wall node are
//   PR_SGT     those of the fill lns_materialize would run for that node
//              (fill_compute through FillSoAIO over the very view it passes;
//              the fill of a node reads only stored arrays); the neighbour's U /
//              V and a cut cell's rho U are the own-cell part (ProbeOwnIO)
//   PR_MECH    lean mechanism state: likewise from the mechanism branch of
//              lns_materialize (the fill's eager mixture closure: bitwise the
//              lazy one's, stepkern.hpp); U, V, rho U by fill_node_pre /
//              fill_node_wall, as probe_row
// Only the listed nodes are filled, and nothing is stored but the scratch
// array and the ring: the step kernels, their argument blocks and the lean
// states are untouched.
#pragma once

#include "../core/load_plan.hpp"
#include "probe_history.hpp"

namespace hf2d {

constexpr int LOADS_BLOCK = 256;        // hf2d_loads_terms: threads per workgroup
constexpr int LOADS_FOLD_WAVES = 16;    // hf2d_loads_fold: wavefronts of its one workgroup
constexpr int LOADS_FOLD_STAGE = 256;   // ... terms a wavefront stages in LDS at a time
constexpr int LOADS_FOLD_GROUP = 32;    // ... terms it reads from LDS ahead of their adds (divides LOADS_FOLD_STAGE)

// U, V and rho U of one node as a download after the step holds them (lean
// N-S / mechanism kinds): the own-cell part of the materialise fill, as
// probe_row; a solid / unset node keeps the generic record's U, V (`out`, the
// materialise's output view) and carries S.
template <int KIND>
HF_HD inline void loads_own_cell(const StepParams& P, const SoA& s, const SoA& out, long idx, real* U, real* V,
                                 real* rhou) {
  const long N = s.N;
  const u64 CT = s.CT[idx];
  if (has_all(CT, CT_SOLID) || !has_all(CT, CT_NODE_IS_SET)) {
    *U = out.U[idx];
    *V = out.V[idx];
    *rhou = s.S[(long)I_RHOU * N + idx];
    return;
  }
  CellLocal c;
  (void)probe_own_cell<KIND>(P, s, idx, c);
  *U = c.U;
  *V = c.V;
  *rhou = c.S[I_RHOU];
}

// What lns_materialize's fill stores for one cell (lean N-S / mechanism
// kinds): `fin` is that fill's input view (sin == pold), `out` its output view,
// whose arrays keep what the fill does not store (fill_cell with store_grad;
// a solid or unset cell is carried early and keeps everything; SGL stores no
// lam_t and no mu_t).  One fill_compute per cell: the load recorder, the wall
// heat recorder and the surface recorder all read their values from this.
struct WallFill {
  real p, Tg, lam, lam_t, mu, mu_t, dUdy, dVdx;
};
template <int KIND>
HF_HD inline WallFill wall_fill_cell(const StepParams& P, const SoA& fin, const SoA& out, long idx) {
  constexpr int MODE = KIND == PR_MECH ? SK_MECH : KIND == PR_SGT ? SK_SGT : SK_SGL;
  constexpr int NSB = KIND == PR_MECH ? 9 : 1;
  const long N = fin.N;
  const int i = (int)(idx / P.ny), j = (int)(idx - (long)i * P.ny);
  FillSoAIO io(fin, fin, idx);
  CellLocal c;
  real mY[NSB], mgx[NSB], mgy[NSB];
  bool early, filled;
  int neg = 0;
  (void)fill_compute<MODE, NSB>(P, io, c, mY, mgx, mgy, fin.mech, fin.nsp, i, j, io.inplace(out), &neg, &early,
                                &filled);
  WallFill w;
  const bool grads = !early && !has_all(c.CT, NT_FC) && P.sm == SM_NS;
  w.p = early ? out.p[idx] : c.p;
  w.Tg = early ? out.Tg[idx] : c.Tg;
  w.lam = early ? out.lam[idx] : c.lam;
  w.lam_t = (early || MODE == SK_SGL) ? out.lam_t[idx] : c.lam_t;
  w.mu = early ? out.mu[idx] : c.mu;
  w.mu_t = (early || MODE == SK_SGL) ? out.mu_t[idx] : c.mu_t;
  w.dUdy = grads ? c.dUdy : out.grad[(long)G_DUDY * N + idx];
  w.dVdx = grads ? c.dVdx : out.grad[(long)G_DVDX * N + idx];
  return w;
}

// p, mu, mu_t, dUdy, dVdx of one node as lns_materialize's fill stores them
struct LoadsWall {
  real p, mu, mu_t, dUdy, dVdx;
};
template <int KIND>
HF_HD inline LoadsWall loads_wall_fill(const StepParams& P, const SoA& fin, const SoA& out, long idx) {
  const WallFill f = wall_fill_cell<KIND>(P, fin, out, idx);
  LoadsWall w;
  w.p = f.p;
  w.mu = f.mu;
  w.mu_t = f.mu_t;
  w.dUdy = f.dUdy;
  w.dVdx = f.dVdx;
  return w;
}

// Value of one term.  `s`: post_step_view's view; `fin` / `out`: the
// materialise fill's views (lean N-S / mechanism kinds only).
template <int KIND>
HF_HD inline real loads_term_value(const StepParams& P, const SoA& s, const SoA& fin, const SoA& out, int kind,
                                   real coef, long c, long c2) {
  const long N = s.N;
  const bool fy = kind == LK_FY;
  if (KIND == PR_GATHER || KIND == PR_LEAN) {
    if (kind == LK_M) return load_term(kind, coef, s.S[(long)I_RHOU * N + c], 0.0, 0.0, 0.0, 0.0);
    if (kind == LK_P) return load_term(kind, coef, s.p[c], 0.0, 0.0, 0.0, 0.0);
    return load_term(kind, coef, 0.0, s.mu[c], s.mu_t[c], s.grad[(long)(fy ? G_DVDX : G_DUDY) * N + c],
                     fy ? s.V[c2] : s.U[c2]);
  } else {
    real U, V, ru;
    if (kind == LK_M) {
      loads_own_cell<KIND>(P, s, out, c, &U, &V, &ru);
      return load_term(kind, coef, ru, 0.0, 0.0, 0.0, 0.0);
    }
    const LoadsWall w = loads_wall_fill<KIND>(P, fin, out, c);
    if (kind == LK_P) return load_term(kind, coef, w.p, 0.0, 0.0, 0.0, 0.0);
    loads_own_cell<KIND>(P, s, out, c2, &U, &V, &ru);
    return load_term(kind, coef, 0.0, w.mu, w.mu_t, fy ? w.dVdx : w.dUdy, fy ? V : U);
  }
}

#ifdef __HIPCC__
// slot: the dt slot lns_materialize's fill would read (lean N-S / mechanism kinds)
template <int KIND>
__global__ __launch_bounds__(LOADS_BLOCK) void hf2d_loads_terms(StepParams P, SoA s, SoA fin, SoA out, LoadsDev L,
                                                                 const DevScalars* sc, int slot) {
  if (KIND != PR_GATHER && KIND != PR_LEAN) apply_dt(P, sc, slot);
  const long t = (long)blockIdx.x * LOADS_BLOCK + threadIdx.x;
  if (t >= L.nterms) return;
  const long c = L.cell[t], c2 = L.cell2[t];
  real v = 0.0;
  if (c >= 0 && c < s.N && c2 >= 0 && c2 < s.N) v = loads_term_value<KIND>(P, s, fin, out, L.kind[t], L.coef[t], c, c2);
  L.scratch[t] = v;
}

// Writes of this wavefront's lanes to LDS before reads of them by its other lanes.
__device__ __forceinline__ void loads_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One wavefront per list (looping when there are more lists than wavefronts).
// The wavefront stages its list's slice of the scratch array in LDS, a block of
// LOADS_FOLD_STAGE terms at a time in coalesced loads (the next block's loads
// are issued before the current one is folded), then every lane reads the
// block's terms in list order (one LDS address for the whole wavefront: a
// broadcast) and adds each into the one running sum, LOADS_FOLD_GROUP reads
// ahead of the dependent adds.  The additions are exactly fold_terms', then
// +0.0 up to the end of the last group: a sum that starts at +0.0 is never
// -0.0, so adding +0.0 leaves every bit of it.  An empty list is +0.0.
__global__ __launch_bounds__(LOADS_FOLD_WAVES* WAVE) void hf2d_loads_fold(LoadsDev L, const DevScalars* sc) {
  __shared__ real stage[LOADS_FOLD_WAVES][LOADS_FOLD_STAGE];
  constexpr int PER = LOADS_FOLD_STAGE / WAVE;
  const int lane = (int)threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / WAVE);   // (the same in every lane: scalar control flow)
  real* mine = stage[wave];
  const unsigned long long n = *L.count;   // (every thread loads before the barrier, thread 0 stores after it)
  const long slot = (long)(n % (unsigned long long)L.cap);
  for (int l = wave; l < L.nlists; l += LOADS_FOLD_WAVES) {
    const long b = L.off[l], e = L.off[l + 1];
    real sum = 0.0;
    real t[PER];
#pragma unroll
    for (int r = 0; r < PER; r++) {
      const long i = b + r * WAVE + lane;
      t[r] = i < e ? L.scratch[i] : (real)0.0;
    }
    for (long q = b; q < e; q += LOADS_FOLD_STAGE) {
#pragma unroll
      for (int r = 0; r < PER; r++) mine[r * WAVE + lane] = t[r];
#pragma unroll
      for (int r = 0; r < PER; r++) {
        const long i = q + LOADS_FOLD_STAGE + r * WAVE + lane;
        t[r] = i < e ? L.scratch[i] : (real)0.0;
      }
      loads_wave_sync();
      const int cnt = (int)(e - q < (long)LOADS_FOLD_STAGE ? e - q : (long)LOADS_FOLD_STAGE);
      for (int k = 0; k < cnt; k += LOADS_FOLD_GROUP) {
        real v[LOADS_FOLD_GROUP];
#pragma unroll
        for (int g = 0; g < LOADS_FOLD_GROUP; g++) v[g] = mine[k + g];
#pragma unroll
        for (int g = 0; g < LOADS_FOLD_GROUP; g++) sum += v[g];
      }
      loads_wave_sync();   // (the block is read before the next one overwrites it)
    }
    if (lane == 0) L.vals[slot * L.nlists + l] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    L.times[slot] = sc->time_part;
    *L.count = n + 1;
  }
}
#endif

}  // namespace hf2d
