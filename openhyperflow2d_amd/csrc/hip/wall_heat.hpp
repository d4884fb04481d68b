// Per-step wall heat recorder on the device (core/wall_heat.hpp): the
// HeatFlux-X profile (Q, Alpha, Cp, St per column) and the HeatFlux-Y profile
// (Q per row) after every sampled step, bit for bit what heat_flux_x_cols /
// heat_flux_y_terms + fold_heat_flux_y give on a field downloaded after that
// step, in a ring, and running statistics of every profile entry.
//
// Up to three launches follow the step on the solver's stream, beside the
// other recorders', so they are captured into the step graphs:
//   hf2d_wallq_tick         one lane: the sampling decision, the weights w, r, W
//                           (stats_tick on the device clock) and the ring row
//   hf2d_wallq_cells<KIND>  one lane per needed cell of the plan (the nodes and
//                           their N1..N4, each once): lam + lam_t, Tg and p of
//                           the cell into scratch
//   hf2d_wallq_fold         one workgroup per list (nx columns, then ny rows):
//                           its nodes' terms from scratch, a block at a time in
//                           parallel, folded in list order by the max-or-first
//                           rule; one lane writes the entries into the ring row
//                           and updates m, M, peak, peak_time in double
// On a step that is not a sample the last two return at once.  A cell's values
// are what a download after the step would hold (KIND: the PR_* kind of
// DeviceSolver::post_step_view):
//   PR_GATHER  generic record, or the lean inviscid arrays after a step that
//              stored T: lam, lam_t, Tg and p are stored per cell (the lean
//              inviscid step and its materialise leave lam, lam_t alone)
//   PR_LEAN    lean inviscid arrays after a plain tile step: Tg = p / R / rho as
//              the probe recorder's row forms it (probe_row)
//   PR_SGL /   lean N-S state: the fill lns_materialize would run, for that cell
//   PR_SGT     only (fill_compute through FillSoAIO over the very views it
//              passes; the fill of a cell reads only stored arrays).  A solid or
//              unset cell is carried early and keeps the stored values; SGL
//              stores no lam_t
//   PR_MECH    lean mechanism state: likewise from the mechanism branch of
//              lns_materialize (the fill's eager mixture closure: bitwise the
//              lazy one's, stepkern.hpp)
// Nothing is stored but the scratch array, the ring and the statistics: the
// step kernels, their argument blocks and the lean states are untouched.
//
// Divisions: the term functions' `/`, which the compiler expands to the IEEE,
// correctly rounded sequence in both precisions (core/wall_heat.hpp); the
// device code is built without contraction.
#pragma once

#include "../core/wall_heat.hpp"
#include "load_history.hpp"

namespace hf2d {

constexpr int WALLQ_BLOCK = 256;   // threads per workgroup of both kernels

// lam + lam_t, Tg, p of one cell.  `s`: post_step_view's view; `fin` / `out`:
// the materialise fill's views (lean N-S / mechanism kinds only).
template <int KIND>
HF_HD inline void wallq_cell(const StepParams& P, const SoA& s, const SoA& fin, const SoA& out, long idx, real* sl,
                             real* Tg, real* p) {
  if (KIND == PR_GATHER || KIND == PR_LEAN) {
    *sl = s.lam[idx] + s.lam_t[idx];
    const u64 ct = s.CT[idx];
    if (KIND == PR_GATHER || has_all(ct, CT_SOLID) || !has_all(ct, CT_NODE_IS_SET)) {
      // (a solid / unset cell is a neighbour only: its Tg and p are never read)
      *Tg = s.Tg[idx];
      *p = s.p[idx];
    } else {
      real row[PROBE_VARS];
      probe_row<KIND>(P, s, idx, row);
      *p = row[0];
      *Tg = row[1];
    }
  } else {
    const WallFill f = wall_fill_cell<KIND>(P, fin, out, idx);
    *sl = f.lam + f.lam_t;
    *Tg = f.Tg;
    *p = f.p;
  }
}

#ifdef __HIPCC__
__global__ __launch_bounds__(64) void hf2d_wallq_tick(WallHeatScalars* w, const DevScalars* sc, int cap) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  StatsScalars t = w->s;
  if (stats_tick(t, sc->time_part - t.t_off)) w->slot = cap > 0 ? (long)((t.samples - 1) % (unsigned long long)cap) : 0;
  w->s = t;
}

// slot: the dt slot lns_materialize's fill would read (lean N-S / mechanism kinds)
template <int KIND>
__global__ __launch_bounds__(WALLQ_BLOCK) void hf2d_wallq_cells(StepParams P, SoA s, SoA fin, SoA out, WallHeatDev L,
                                                                 const DevScalars* sc, int slot) {
  if (!L.ring.sc->s.sample) return;
  if (KIND != PR_GATHER && KIND != PR_LEAN) apply_dt(P, sc, slot);
  const long t = (long)blockIdx.x * WALLQ_BLOCK + threadIdx.x;
  if (t >= L.ncells) return;
  const long c = L.cells[t];
  real sl = 0.0, Tg = 0.0, p = 0.0;
  if (c >= 0 && c < s.N) wallq_cell<KIND>(P, s, fin, out, c, &sl, &Tg, &p);
  L.scratch[t] = sl;
  L.scratch[L.ncells + t] = Tg;
  L.scratch[2 * L.ncells + t] = p;
}

// One workgroup per list.  A term (five gathers through the plan and three
// divisions) depends on no other term, so the workgroup's lanes form
// WALLQ_BLOCK terms of the list at a time, in parallel, into LDS; the fold
// itself is sequential by its rule (the test on the old Q), so after each
// block the first wavefront walks the block in list order, every lane reading
// the same LDS word (a broadcast) and carrying the same Q and Alpha.  One lane
// folding its whole list on its own, terms included, took 750 us per step on
// the resonator's 1760-node row (profiles/wall_heat.md).  An empty list is +0.0.
__global__ __launch_bounds__(WALLQ_BLOCK) void hf2d_wallq_fold(WallHeatDev L, const DevScalars* sc) {
  __shared__ real tq[WALLQ_BLOCK], ta[WALLQ_BLOCK];
  __shared__ real last[2];   // Cp, St of the list's last node
  const WallHeatScalars* w = L.ring.sc;
  if (!w->s.sample) return;
  const int l = (int)blockIdx.x, tid = (int)threadIdx.x;   // (the grid has nx + ny workgroups)
  const int b = L.off[l], e = L.off[l + 1];
  const bool col = l < L.nx;
  const real *sl = L.scratch, *sT = sl + L.ncells, *sp = sT + L.ncells;
  real Q = 0.0, Al = 0.0;
  for (int q0 = b; q0 < e; q0 += WALLQ_BLOCK) {
    const int t = q0 + tid;
    if (t < e) {
      const int* c = L.node5 + 5 * (long)L.list[t];
      const real lam_eff = wall_heat_lam_eff(sl[c[0]], sl[c[1]], sl[c[2]], sl[c[3]], sl[c[4]]);
      if (col) {
        const WallHeatXTerm x = wall_heat_x_term(L.K, lam_eff, sT[c[0]], sp[c[0]]);
        tq[tid] = x.q;
        ta[tid] = x.alpha;
        if (t == e - 1) {
          last[0] = x.cp;
          last[1] = x.st;
        }
      } else {
        tq[tid] = wall_heat_q(L.K, lam_eff, sT[c[0]], L.K.dx);
      }
    }
    __syncthreads();
    if (tid < WAVE) {   // (the whole first wavefront: uniform control flow, the same values in every lane)
      const int cnt = e - q0 < WALLQ_BLOCK ? e - q0 : WALLQ_BLOCK;
      if (col) {
#pragma unroll 8
        for (int k = 0; k < cnt; k++) wall_heat_fold_x(Q, Al, tq[k], ta[k]);
      } else {
#pragma unroll 8
        for (int k = 0; k < cnt; k++) wall_heat_fold_y(Q, tq[k]);
      }
    }
    __syncthreads();   // (the block is read before the next one overwrites it; `last` is visible)
  }
  if (tid != 0) return;
  const real out[WALL_HEAT_X] = {Q, Al, (col && e > b) ? last[0] : (real)0.0, (col && e > b) ? last[1] : (real)0.0};
  const long ne = (long)WALL_HEAT_X * L.nx + L.ny, slot = w->slot;
  const double t = sc->time_part, wt = w->s.w, r = w->s.r;
  const bool first = w->s.samples == 1;
  double *m = L.ring.stat, *M = m + ne, *pk = M + ne, *pt = pk + ne;
#pragma unroll
  for (int k = 0; k < WALL_HEAT_X; k++) {
    if (k > 0 && !col) break;
    const int en = wall_heat_entry(L.nx, l, k);
    if (L.ring.cap > 0) L.ring.vals[slot * ne + en] = out[k];
    if (L.ring.statistics) wall_heat_stat(wt, r, t, first, (double)out[k], m[en], M[en], pk[en], pt[en]);
  }
  if (l == 0 && L.ring.cap > 0) L.ring.times[slot] = t;
}
#endif

}  // namespace hf2d
