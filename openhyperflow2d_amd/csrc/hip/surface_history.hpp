// Per-step surface recorder on the device (core/surface_plan.hpp): p, Cp, T,
// tau_x, tau_y, Cf_x, Cf_y, q_y, q_x and St of every listed wall node after
// every sampled step, bit for bit what surface_values gives on a field
// downloaded after that step, in a ring, and running statistics of every
// (variable, node) entry.
//
// Three launches follow the step on the solver's stream, beside the other
// recorders', so they are captured into the step graphs:
//   hf2d_wallq_tick        (wall_heat.hpp) on this recorder's own scalars: the
//                          sampling decision, the weights and the ring row
//   hf2d_surf_cells<KIND>  one lane per needed cell of the plan (each once): by
//                          the cell's mask p, Tg, lam + lam_t, mu, mu_t, dUdy,
//                          dVdx, U, V into the scratch planes
//   hf2d_surf_nodes        one lane per list position: gathers from scratch
//                          through the plan's indices, forms the ten values and
//                          stores them at [slot][var][node] (coalesced over the
//                          node), updates m, M, peak, peak_time in double; lane
//                          0 of workgroup 0 writes the sample's time
// On a step that is not a sample the last two return at once.  No fold and no
// atomics: every entry has one writer.
//
// A cell's values are what a download after the step would hold (KIND: the
// PR_* kind of DeviceSolver::post_step_view):
//   PR_GATHER / PR_LEAN  the stored arrays; p and Tg of a node by probe_row on
//                        the lean inviscid arrays (as wallq_cell)
//   PR_SGL / PR_SGT /    a node: one materialise fill for that cell
//   PR_MECH              (wall_fill_cell, load_history.hpp); a friction
//                        neighbour: the own-cell part (loads_own_cell); a cell
//                        that gives lam + lam_t only: wallq_cell
// Nothing is stored but the scratch planes, the ring and the statistics.
#pragma once

#include "../core/surface_plan.hpp"
#include "wall_heat.hpp"

namespace hf2d {

constexpr int SURF_BLOCK = 256;   // threads per workgroup of both kernels

// The scratch planes' values of one needed cell, by its mask; what the mask
// does not ask for is +0.0.  `s`: post_step_view's view; `fin` / `out`: the
// materialise fill's views (lean N-S / mechanism kinds only).
template <int KIND>
HF_HD inline void surf_cell(const StepParams& P, const SoA& s, const SoA& fin, const SoA& out, long idx, int mask,
                            real v[SURFACE_PLANES]) {
  const long N = s.N;
#pragma unroll
  for (int q = 0; q < SURFACE_PLANES; q++) v[q] = 0.0;
  if (mask & SC_NODE) {
    if (KIND == PR_GATHER || KIND == PR_LEAN) {
      wallq_cell<KIND>(P, s, fin, out, idx, &v[SP_SL], &v[SP_T], &v[SP_P]);
      v[SP_MU] = s.mu[idx];
      v[SP_MUT] = s.mu_t[idx];
      v[SP_DUDY] = s.grad[(long)G_DUDY * N + idx];
      v[SP_DVDX] = s.grad[(long)G_DVDX * N + idx];
    } else {
      const WallFill f = wall_fill_cell<KIND>(P, fin, out, idx);
      v[SP_P] = f.p;
      v[SP_T] = f.Tg;
      v[SP_SL] = f.lam + f.lam_t;
      v[SP_MU] = f.mu;
      v[SP_MUT] = f.mu_t;
      v[SP_DUDY] = f.dUdy;
      v[SP_DVDX] = f.dVdx;
    }
  } else if (mask & SC_LAM) {
    real Tg, p;
    wallq_cell<KIND>(P, s, fin, out, idx, &v[SP_SL], &Tg, &p);
  }
  if (mask & (SC_U | SC_V)) {
    if (KIND == PR_GATHER || KIND == PR_LEAN) {
      v[SP_U] = s.U[idx];
      v[SP_V] = s.V[idx];
    } else {
      real ru;
      loads_own_cell<KIND>(P, s, out, idx, &v[SP_U], &v[SP_V], &ru);
    }
  }
}

#ifdef __HIPCC__
// slot: the dt slot lns_materialize's fill would read (lean N-S / mechanism kinds)
template <int KIND>
__global__ __launch_bounds__(SURF_BLOCK) void hf2d_surf_cells(StepParams P, SoA s, SoA fin, SoA out, SurfaceDev L,
                                                               const DevScalars* sc, int slot) {
  if (!L.ring.sc->s.sample) return;
  if (KIND != PR_GATHER && KIND != PR_LEAN) apply_dt(P, sc, slot);
  const long t = (long)blockIdx.x * SURF_BLOCK + threadIdx.x;
  if (t >= L.ncells) return;
  const long c = L.cells[t];
  real v[SURFACE_PLANES];
#pragma unroll
  for (int q = 0; q < SURFACE_PLANES; q++) v[q] = 0.0;
  if (c >= 0 && c < s.N) surf_cell<KIND>(P, s, fin, out, c, (int)L.mask[t], v);
#pragma unroll
  for (int q = 0; q < SURFACE_PLANES; q++) L.scratch[(long)q * L.ncells + t] = v[q];
}

// The grid has at least one workgroup, also for a plan without nodes: the
// sample's time is recorded all the same.
__global__ __launch_bounds__(SURF_BLOCK) void hf2d_surf_nodes(SurfaceDev L, const DevScalars* sc) {
  const WallHeatScalars* w = L.ring.sc;
  if (!w->s.sample) return;
  const long n = (long)blockIdx.x * SURF_BLOCK + threadIdx.x;
  const long slot = w->slot;
  const double t = sc->time_part;
  if (n == 0 && L.ring.cap > 0) L.ring.times[slot] = t;
  if (n >= L.nnodes) return;
  real out[SURFACE_NVARS];
  surface_node(L.K, L.idx, L.bits, L.scratch, L.ncells, n, out);
  const long ne = (long)SURFACE_NVARS * L.nnodes;
  const double wt = w->s.w, r = w->s.r;
  const bool first = w->s.samples == 1;
  double *m = L.ring.stat, *M = m + ne, *pk = M + ne, *pt = pk + ne;
#pragma unroll
  for (int v = 0; v < SURFACE_NVARS; v++) {
    const long e = (long)v * L.nnodes + n;
    if (L.ring.cap > 0) L.ring.vals[slot * ne + e] = out[v];
    if (L.ring.statistics) wall_heat_stat(wt, r, t, first, (double)out[v], m[e], M[e], pk[e], pt[e]);
  }
}
#endif

}  // namespace hf2d
