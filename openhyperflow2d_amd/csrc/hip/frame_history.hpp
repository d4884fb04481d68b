// Per-step frame recorder on the device (core/frame_rule.hpp): the armed
// variables of FRAME_VARS on the cells of a strided region after every sampled
// step, bit for bit what frame_eval gives on a field downloaded after that
// step, in a ring of frames.  The first observer that reads a cell's
// neighbours.
//
// Up to three launches follow the step on the solver's stream, beside the
// other recorders', so they are captured into the step graphs:
//   hf2d_wallq_tick         (wall_heat.hpp) on this recorder's own scalars: the
//                           sampling decision and the ring slot
//   hf2d_frame_rows<KIND>   one lane per cell of the geometry's box (the region,
//                           with a stencil variable armed dilated by one cell
//                           and clipped to the grid): the probe_row of a gas
//                           cell into the five scratch planes.  A non-gas cell
//                           is skipped before probe_row (a solid node must not
//                           enter the lean N-S fill, as in hf2d_stats_accum),
//                           and the store kernel never reads its planes.  Every
//                           row is evaluated once per sample -- on the lean N-S
//                           state a row is one fill_compute, which is why the
//                           stencil kernel does not call probe_row five times
//   hf2d_frame_store        not templated on the kind: one lane per output
//                           cell, consecutive lanes on consecutive j.  j is the
//                           fastest index of the x-major planes, so the centre
//                           and the S / N loads are contiguous and the W / E
//                           loads are contiguous one box row away.  It reads CT
//                           and the scratch rows of the cell and its four
//                           neighbours, runs frame_cell for the armed variables
//                           (a wave-uniform bit mask) and stores
//                           [slot][var][a][b], coalesced over b; lane 0 of
//                           workgroup 0 writes the sample's time
// On a step that is not a sample the last two return at once.  No LDS tiling:
// a scratch value is read by at most five lanes, which L2 serves.  Nothing is
// stored but the scratch planes and the ring: the step kernels, their argument
// blocks and the lean states are untouched.
#pragma once

#include "../core/frame_rule.hpp"
#include "wall_heat.hpp"

namespace hf2d {

constexpr int FRAME_BLOCK = 256;   // threads per workgroup of both kernels
static_assert(FRAME_ROW == PROBE_VARS, "the frame's row is the probe recorder's");

#ifdef __HIPCC__
template <int KIND>
__global__ __launch_bounds__(FRAME_BLOCK) void hf2d_frame_rows(StepParams P, SoA s, FrameDev L) {
  if (!L.ring.sc->s.sample) return;
  const FrameGeom& G = L.G;
  const long t = (long)blockIdx.x * FRAME_BLOCK + threadIdx.x;
  if (t >= G.nbox()) return;
  const int dnj = G.dj1 - G.dj0;
  const int a = (int)(t / dnj);
  const int i = G.di0 + a, j = G.dj0 + (int)(t - (long)a * dnj);
  const long idx = (long)(i + G.ioff) * G.ny + j;
  if (idx < 0 || idx >= s.N) return;
  if (!frame_gas(s.CT[idx])) return;   // (before probe_row)
  real row[PROBE_VARS];
  probe_row<KIND>(P, s, idx, row);
  const long nb = G.nbox();
#pragma unroll
  for (int v = 0; v < FRAME_ROW; v++) L.scratch[(long)v * nb + t] = row[v];
}

// The grid has at least one workgroup, also for a strip that owns no output
// column: the sample's time is recorded all the same.
__global__ __launch_bounds__(FRAME_BLOCK) void hf2d_frame_store(FrameDev L, const u64* CT, long N, const DevScalars* sc) {
  const WallHeatScalars* w = L.ring.sc;
  if (!w->s.sample) return;
  const FrameGeom& G = L.G;
  const long t = (long)blockIdx.x * FRAME_BLOCK + threadIdx.x;
  const long slot = w->slot;
  if (t == 0) L.ring.times[slot] = sc->time_part;
  const long nc = G.ncells();
  if (t >= nc) return;
  const int a = (int)(t / G.nj), b = (int)(t - (long)a * G.nj);
  const int i = G.i0 + a * G.si, j = G.j0 + b * G.sj;
  const long idx = (long)(i + G.ioff) * G.ny + j;
  real out[FRAME_NVARS];
#pragma unroll
  for (int v = 0; v < FRAME_NVARS; v++) out[v] = 0.0;
  if (idx >= 0 && idx < N && frame_gas(CT[idx])) {
    const bool st = (G.mask & FRAME_GRAD_MASK) != 0;   // (else the box is the region itself: no neighbour is read)
    const bool hasW = st && i > 0 && frame_gas(CT[idx - G.ny]), hasE = st && i + 1 < G.nx && frame_gas(CT[idx + G.ny]);
    const bool hasS = st && j > 0 && frame_gas(CT[idx - 1]), hasN = st && j + 1 < G.ny && frame_gas(CT[idx + 1]);
    const long nb = G.nbox(), c = G.box_at(i, j);
    const int dnj = G.dj1 - G.dj0;
    const real* S = L.scratch;
    auto q = [&](int n, int v) {
      const long o = n == FN_W ? -(long)dnj : n == FN_E ? (long)dnj : n == FN_S ? -1L : n == FN_N ? 1L : 0L;
      return S[(long)v * nb + c + o];
    };
    frame_cell(G.mask, hasW, hasE, hasS, hasN, G.dx, G.dy, q, out);
  }
  real* o = L.ring.vals + slot * ((long)G.nvars * nc) + t;
  // (constant indices only: out stays in registers)
#pragma unroll
  for (int k = 0; k < FRAME_NVARS; k++) {
    if (k >= G.nvars) break;
    const int var = G.var[k];
    real x = out[0];
#pragma unroll
    for (int v = 1; v < FRAME_NVARS; v++) x = var == v ? out[v] : x;
    o[(long)k * nc] = x;
  }
}
#endif

}  // namespace hf2d
