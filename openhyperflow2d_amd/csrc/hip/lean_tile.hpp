// Inviscid lean tile kernels (lean_euler.hpp on LDS tiles):
//   lean_tile_body         the tile step; hf2d_lean_tile and its _fx (fused
//                          exchange), _tr (phase trace) and _nt (128 / 64
//                          threads) forms
// The fused exchange's types and device functions are in dev_common.hpp.
// Included by step_tile.hip only.
#pragma once

#include "../core/lean_euler.hpp"
#include "dev_common.hpp"

namespace hf2d {

// Single-GPU last step of a host call (StepParams::host_sc): the last
// workgroup to finish copies the slot's dt (word + shards) and the error flag
// into the pinned host mirror (workgroup 0's head wrote time_part / dt_lag
// there), so DeviceSolver::sync_scalars only waits for the stream: no
// hf2d_scalars_out launch and its completion round trip (13 us of an idle
// step(0) call, tools/call_overhead.py).  Completion count as fx_tail.
__device__ __forceinline__ void host_mirror_tail(const StepParams& P, DevScalars* sc, int slot_next) {
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  vm_drain();   // lane 0's dt atomic
  int last = 0;
  if (lane == 0) {
    const unsigned G = gridDim.x, sh = blockIdx.x % DT_SHARDS;
    const unsigned pop = (G - sh + DT_SHARDS - 1) / DT_SHARDS, nsh = G < DT_SHARDS ? G : DT_SHARDS;
    unsigned* cs = P.host_done + sh * FX_DONE_STRIDE;
    unsigned* ct = P.host_done + DT_SHARDS * FX_DONE_STRIDE;
    if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pop - 1) {
      __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsh - 1) {
        __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = 1;
      }
    }
  }
  if (!__shfl(last, 0, WAVE)) return;
  unsigned long long b = ~0ull;
  if (lane < DT_SHARDS) b = __hip_atomic_load(&sc->dt_sh[slot_next][lane][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane == DT_SHARDS) b = __hip_atomic_load(&sc->dt_bits[slot_next], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (P.dt_fold) {
    // the step's MIN into the slot's word: the next step reads one word
    // (StepParams::dt_read = 2) instead of the word and 16 shards
    unsigned long long m = b;
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) m = dt_bits_min(m, (unsigned long long)__shfl_xor((long long)m, off, WAVE));
    m = (unsigned long long)__shfl((long long)m, 0, WAVE);
    if (lane == DT_SHARDS) {
      b = m;
      __hip_atomic_store(&sc->dt_bits[slot_next], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (!P.host_sc) return;
  DevScalars* h = static_cast<DevScalars*>(P.host_sc);
  if (lane <= DT_SHARDS) (lane < DT_SHARDS ? h->dt_sh[slot_next][lane][0] : h->dt_bits[slot_next]) = b;
  if (lane == DT_SHARDS + 1) h->neg_T = __hip_atomic_load(&sc->neg_T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// (workgroup 0's head, thread 0, after its updates of the slot words)
__device__ __forceinline__ void host_mirror_head(const StepParams& P, const DevScalars* sc, int slot_next) {
  DevScalars* h = static_cast<DevScalars*>(P.host_sc);
  h->time_part = sc->time_part;
  h->dt_lag[slot_next] = sc->dt_lag[slot_next];
}

// LDS-tiled lean step (lean_euler.hpp: lean_tile_stage / TileIO).
// In-kernel phase trace (TR): thread 0 of every workgroup records the
// 100 MHz s_memrealtime clock at entry, after the LDS staging barrier, when
// its own wave finished computing, after the block dt reduction barrier and
// after the dt atomic, plus the HW_ID / XCC_ID registers (DeviceSolver::trace_tile).
constexpr int TILE_TRACE_WORDS = 8;
#ifndef HF2D_TILE_STAGGER
#define HF2D_TILE_STAGGER 1
#endif
constexpr int LDS_PER_CU = 160 * 1024;

// Batched staging of a single-gas tile (device form of lean_tile_stage<true>,
// same LDS layout, same skipped slots, same values).  Thread t owns the slots
// t, t + NT, ..., K = ceil(NC / NT) of them (LeanTile::stage, set by the host):
// lean_stage_issue starts all K x 7 loads into registers in one unrolled
// block, lean_stage_write stores them to LDS.  Between the two the kernel
// issues what else it has to load, so a wave pays one round trip for its
// staging instead of one per pass of lean_tile_stage's loop (whose trip count
// is a run-time value: its second pass loads only after the first has
// arrived and been written).
// Largest K a kernel of nt threads and cpt cells per thread stages this way:
// the largest at which every variant of it keeps the occupancy step it has
// with the loop alone and spills nothing to scratch; beyond it the kernel runs
// the loop.  3 for all of them: the K x 14 staging VGPRs are live where the
// step's own arithmetic is not yet, and 42 fit under every kernel's peak (the
// plain one-cell kernels stay at 95 VGPRs, 5 waves per SIMD); with 4 the
// one-cell kernels go 95 -> 107 (5 -> 4 waves) and the two-cell fused-exchange
// ones 121 -> 129 (4 -> 3), profiles/tile_stage_batch.md.  The geometries the
// autotune picks need 2 (64 x 1 x 16, 128 x 1 x 8, 256 x 1) or 3 (256 x 2).
__host__ __device__ constexpr int lean_stage_kmax(int nt, int cpt) {
  (void)nt;
  (void)cpt;
  return 3;
}
constexpr int LEAN_STAGE_KTOP = 3;   // largest K lean_tile_body dispatches
template <int KM>
struct LeanStaged {   // (room for KM slots; a tile of K < KM uses the first K)
  real v[KM > 0 ? KM : 1][LEAN_TILE_FIELDS_SG];
  int c[KM > 0 ? KM : 1];   // LDS slot, < 0: not staged (halo corner, outside the grid, beyond NC)
};
template <int K, int NT, int KM>
__device__ __forceinline__ void lean_stage_issue(const StepParams& P, const LeanSoA& L, const LeanTile& T, int i0,
                                                 int j0, LeanStaged<KM>& s) {
  static_assert(K <= KM, "slots");
  const long N = L.N;
#pragma unroll
  for (int k = 0; k < K; k++) {
    const int c = (int)threadIdx.x + k * NT;
    // (the division per slot: lean_tile_stage)
    const int ii = c / T.W - 1, jj = c - (ii + 1) * T.W - 1;
    const bool xh = ii < 0 || ii >= T.TI, yh = jj < 0 || jj >= T.TJ;
    const int gi = i0 + ii, gj = j0 + jj;
    const bool skip = c >= T.NC || (xh && yh) || gi < 0 || gi >= P.nx || gj < 0 || gj >= P.ny;
    s.c[k] = skip ? -1 : c;
    if (!skip) {
      const long g = (long)gi * P.ny + gj;
#pragma unroll
      for (int f = 0; f < 4; f++) s.v[k][f] = L.Sin[f * N + g];
      s.v[k][4] = L.Uin[g];
      s.v[k][5] = L.Vin[g];
      s.v[k][6] = L.Pin[g];
    }
  }
}
template <int K, int KM>
__device__ __forceinline__ void lean_stage_write(const LeanTile& T, const LeanStaged<KM>& s, real* lds) {
  static_assert(K <= KM, "slots");
#pragma unroll
  for (int k = 0; k < K; k++)
    if (s.c[k] >= 0)
#pragma unroll
      for (int f = 0; f < LEAN_TILE_FIELDS_SG; f++) lds[f * T.NC + s.c[k]] = s.v[k][f];
}

// The species pack's AirTable in a single-gas tile's LDS, behind the staged
// fields at the next 8-byte boundary: thread t < AIR_TABLE_WORDS carries word
// t.  The load has no condition (threads beyond the block read its word 0, and
// a pack in mode 0 has a block too, which nothing reads), so it is one more
// load of the staging batch and the backend still counts what is in flight;
// it is issued with the tile's own loads and stored to LDS with them, in
// front of the staging barrier.
HF_HD constexpr size_t air_table_lds_offset(int NC) {
  return ((size_t)LEAN_TILE_FIELDS_SG * NC * sizeof(real) + 7) & ~(size_t)7;
}
constexpr size_t AIR_TABLE_LDS_BYTES = sizeof(AirTable);
__device__ __forceinline__ unsigned long long air_table_issue(const SpeciesProps* sp) {
  const unsigned t = threadIdx.x < (unsigned)AIR_TABLE_WORDS ? threadIdx.x : 0u;
  return reinterpret_cast<const unsigned long long*>(air_table_of(sp))[t];
}
__device__ __forceinline__ void air_table_write(AirTable* tab, unsigned long long w) {
  if (threadIdx.x < (unsigned)AIR_TABLE_WORDS) reinterpret_cast<unsigned long long*>(tab)[threadIdx.x] = w;
}

// Workgroup 0's once-per-step updates of the scalars, after P.dt is known
// (MIRROR: the host mirror's part, host_mirror_head).
template <bool MIRROR, bool FX>
__device__ __forceinline__ void lean_tile_wg0_head(const StepParams& P, DevScalars* sc, int slot, int slot_next,
                                                   const FusedX& X, unsigned long long seq_prev) {
  if (threadIdx.x < WAVE) {
    // lagged dt with the fold deferred (X.defer): the previous step's tail
    // waited for the two neighbours only; the other ranks' dt of that step
    // is folded here, one step later, by this wavefront (one peer per lane)
    double fold = 1.0;
    if (FX && X.defer && P.lag_dt && seq_prev > 0) {
      bool ok;
      fold = p2p_wait_wave(X, seq_prev, sc, [](int) { return true; }, true, (int)(seq_prev & 1), &ok);
    }
    if (threadIdx.x == 0) {
      dt_reset(sc, slot_reset(slot));
      lag_head(P, sc, slot, slot_next, fold);
      sc->dt_bits[slot] = d_to_bits(P.dt);   // folded (later kernels of the step read the word)
      sc->time_part += P.dt;
      scenario_next(P, sc, slot, slot_next);
      if (MIRROR && P.host_sc) host_mirror_head(P, sc, slot_next);
    }
  }
}

// NT: threads per workgroup (BLOCK, or 128 / 64 for the small strips of a
// multi-GPU run: at 250 x 200 cells per GPU a 256-thread tiling leaves ~50 of
// the 256 CUs without a workgroup, and the step is one workgroup's
// load -> compute -> reduce chain)
template <bool RES, bool OUT, bool SG, int CPT, bool FX = false, bool TR = false, int NT = BLOCK>
__device__ __forceinline__ void lean_tile_body(StepParams& P, const LeanSoA& L, const LeanTile& T, DevScalars* sc,
                                               int slot, int slot_next, int serial, ResidualPack* partials,
                                               const FusedX& X = FusedX{}, unsigned long long* trace = nullptr,
                                               int part = 0) {
  extern __shared__ real lds[];
  unsigned long long tr[5];
  if (TR) tr[0] = rt_clock();
  // (compiled into the single-gas two-cell kernel only: the mere presence of
  // this block made the multi-gas one-cell kernel 3x slower on the triple
  // point, 340 -> 1030 us, even with stagger 0)
  if (HF2D_TILE_STAGGER && SG && CPT == 2 && !FX && NT == BLOCK && P.stagger != 0) {
    // staggered start: every workgroup of a step is resident at once, so
    // without it they all stage together (HBM saturated, VALUs idle) and
    // then all compute (HBM idle); later dispatch rounds start loading while
    // the earlier ones compute
    // (rounds beyond the 4th are dispatched as earlier workgroups retire:
    // no wait for them)
    // (stagger > 0: whole rounds of stagger_wgs workgroups; < 0: a linear
    // ramp of the same slope over the first four rounds)
    const unsigned r = blockIdx.x / (unsigned)P.stagger_wgs;
    if (r < 4 && (P.stagger < 0 || r > 0)) {
      const unsigned long long d = P.stagger > 0 ? (unsigned long long)r * (unsigned)P.stagger
                                                 : (unsigned long long)blockIdx.x * (unsigned)(-P.stagger) /
                                                       (unsigned)P.stagger_wgs;
      const unsigned long long t0 = rt_clock();
      while (rt_clock() - t0 < d) __builtin_amdgcn_s_sleep(2);
    }
  }
  // (fused exchange: the strip's edge tile columns first -- they push the
  // halo and stage the ghost columns from the mailbox)
  const unsigned b = (FX && X.edge_first) ? tile_edge_first(xcd_remap(blockIdx.x, gridDim.x), T)
                                          : tile_of_part(xcd_remap(blockIdx.x, gridDim.x), part, T);
  unsigned long long seq_prev = 0;
  if (FX) seq_prev = *X.seq;
  // (single gas: the dt read is only started here, and workgroup 0's head,
  // which needs P.dt, runs after the staging barrier)
  unsigned long long dtb = 0;
  if (SG) dtb = dt_tile_issue(P, sc, slot);
  else apply_dt(P, sc, slot, true);
  if (!SG && b == 0) lean_tile_wg0_head<OUT && !RES && !FX, FX>(P, sc, slot, slot_next, X, seq_prev);
  int i[CPT], j[CPT], c[CPT], i0, j0;
  bool mine[CPT];
  // own-cell global inputs first, so they are in flight during the staging
  LeanOwn own[CPT];
#pragma unroll
  for (int q = 0; q < CPT; q++) {
    mine[q] = lean_tile_cell(P, T, (int)b, (int)threadIdx.x, &i[q], &j[q], &c[q], &i0, &j0, q);
    if (mine[q]) {
      if (SG) lean_load_own_flags(L, (long)i[q] * P.ny + j[q], own[q]);
      else lean_load_own<TileIO<SG>::NE>(L, (long)i[q] * P.ny + j[q], own[q]);
    }
  }
  // staged from the state arrays alone (not an edge tile of a fused exchange)
  const bool plain = !FX || seq_prev == 0 || (X.skip & 4) || (i0 - 1 > P.i0 - 1 && i0 + T.TI < P.i1);
  // (single gas: the AirTable travels with whichever staging follows)
  static_assert(NT >= AIR_TABLE_WORDS, "one AirTable word per thread");
  AirTable* tab = nullptr;
  unsigned long long tabw = 0;
  if constexpr (SG) {
    extern __shared__ double lds8[];   // (the same LDS; 8-byte aligned in the FP32 build too)
    tab = reinterpret_cast<AirTable*>(reinterpret_cast<char*>(lds8) + air_table_lds_offset(T.NC));
    tabw = air_table_issue(P.species);
  }
  if (SG && plain) {
    // Ordered so that a wave's independent loads overlap: the dt word and
    // the own cells' CT / lb are in flight; the whole staging is issued next,
    // then -- the only wait in front of them is the one for CT -- the own
    // cells' beta / CP / R / kk; dt is finished while those travel, and the
    // LDS stores come last.  (Common code between the two K dispatches, not
    // a copy per K: the compiler hoists the CT test out of per-K copies to
    // in front of the staging loads.)
    constexpr int KMAX = lean_stage_kmax(NT, CPT);
    static_assert(KMAX <= LEAN_STAGE_KTOP, "lean_tile_body dispatches K <= LEAN_STAGE_KTOP");
    LeanStaged<KMAX> s;
    const int K = T.stage;   // (beyond KMAX the host sends 0)
    if (KMAX >= 2 && K == 2) lean_stage_issue<(KMAX >= 2 ? 2 : 0), NT>(P, L, T, i0, j0, s);
    else if (KMAX >= 3 && K == 3) lean_stage_issue<(KMAX >= 3 ? 3 : 0), NT>(P, L, T, i0, j0, s);
#pragma unroll
    for (int q = 0; q < CPT; q++) {
      // (the Euler step tests bits of CT's low word only)
      keep_whole(own[q].CT);
      if (mine[q]) lean_load_own_rest<4>(L, (long)i[q] * P.ny + j[q], own[q]);
    }
    dt_tile_finish(P, dtb);
    if (KMAX >= 2 && K == 2) lean_stage_write<(KMAX >= 2 ? 2 : 0)>(T, s, lds);
    else if (KMAX >= 3 && K == 3) lean_stage_write<(KMAX >= 3 ? 3 : 0)>(T, s, lds);
    else lean_tile_stage<true>(P, L, T, i0, j0, lds, threadIdx.x, NT);
  } else if (plain) {
    lean_tile_stage<SG>(P, L, T, i0, j0, lds, threadIdx.x, NT);
  } else {
    if (SG) {
#pragma unroll
      for (int q = 0; q < CPT; q++)
        if (mine[q]) lean_load_own_rest<4>(L, (long)i[q] * P.ny + j[q], own[q]);
      dt_tile_finish(P, dtb);
    }
    // edge tile: the ghost column comes from the mailbox of parity seq_prev
    constexpr int NF = SG ? LEAN_TILE_FIELDS_SG : LEAN_TILE_FIELDS;
    const int pp = (int)(seq_prev & 1);
    const real* mbL = X.my_recv + ((long)pp * 2) * X.cap;
    const real* mbR = X.my_recv + ((long)pp * 2 + 1) * X.cap;
    const long N = L.N;
    constexpr int NS = SG ? 4 : 4 + NCOMP;
    constexpr int FU = SG ? 4 : 10;
    for (int c = threadIdx.x; c < T.NC; c += NT) {
      const int ii = c / T.W - 1, jj = c - (ii + 1) * T.W - 1;
      const bool xh = ii < 0 || ii >= T.TI, yh = jj < 0 || jj >= T.TJ;
      const int gi = i0 + ii, gj = j0 + jj;
      if ((xh && yh) || gi < 0 || gi >= P.nx || gj < 0 || gj >= P.ny) continue;
      const bool gl = (X.sides & 1) && gi == P.i0 - 1, gr = (X.sides & 2) && gi == P.i1;
      if (gl || gr) {
        const real* mb = gl ? mbL : mbR;
#pragma unroll
        for (int f = 0; f < NF; f++) lds[f * T.NC + c] = p2p_load(mb + (long)f * P.ny + gj);
        continue;
      }
      const long g = (long)gi * P.ny + gj;
#pragma unroll
      for (int f = 0; f < NS; f++) lds[f * T.NC + c] = L.Sin[f * N + g];
      if (!SG)
#pragma unroll
        for (int f = 0; f < NCOMP; f++) lds[(4 + NCOMP + f) * T.NC + c] = L.Pin_s[f * N + g];
      lds[FU * T.NC + c] = L.Uin[g];
      lds[(FU + 1) * T.NC + c] = L.Vin[g];
      lds[(FU + 2) * T.NC + c] = L.Pin[g];
    }
  }
  if constexpr (SG) air_table_write(tab, tabw);
  __syncthreads();
  if (SG && b == 0) lean_tile_wg0_head<OUT && !RES && !FX, FX>(P, sc, slot, slot_next, X, seq_prev);
  // (raising the wave priority here for the compute phase, s_setprio 2,
  // measured no change: headline 26.9 - 27.2 us either way, triple point
  // 350 - 353 us)
  if (TR) tr[1] = rt_clock();
  ResidualPack r;
  if (RES) residual_begin(r);
  double dtl = 1.0;
  int neg = 0;
#pragma unroll
  for (int q = 0; q < CPT; q++) {
    if (mine[q]) {
      TileIO<SG> io(L, (long)i[q] * P.ny + j[q], lds, T.NC, T.W, c[q]);
      if constexpr (SG) {
        io.tab = tab;
        io.table = T.table;
      }
      dtl = fmin(dtl, lean_cell<RES, OUT>(P, L, io, own[q], i[q], j[q], r, &neg));
      if (FX) {
        const bool pl = (X.sides & 1) && i[q] == P.i0, pr = (X.sides & 2) && i[q] == P.i1 - 1;
        if ((pl || pr) && !(X.skip & 2)) {   // new lean state of an edge cell -> the neighbour's mailbox of parity seq_prev + 1
          constexpr int NF = SG ? LEAN_TILE_FIELDS_SG : LEAN_TILE_FIELDS;
          constexpr int NS = SG ? 4 : 4 + NCOMP;
          const int pn = (int)((seq_prev + 1) & 1);
          real* mb = pl ? X.peer_recv_l + ((long)pn * 2 + 1) * X.cap : X.peer_recv_r + ((long)pn * 2) * X.cap;
          const long N = L.N, g = (long)i[q] * P.ny + j[q];
          real v[NF];
#pragma unroll
          for (int f = 0; f < NS; f++) v[f] = L.Sout[f * N + g];
          if (!SG)
#pragma unroll
            for (int f = 0; f < NCOMP; f++) v[4 + NCOMP + f] = L.Pout_s[f * N + g];
          v[NF - 3] = L.Uout[g];
          v[NF - 2] = L.Vout[g];
          v[NF - 1] = L.Pout[g];
#pragma unroll
          for (int f = 0; f < NF; f++) p2p_store(mb + (long)f * P.ny + j[q], v[f]);
          vm_drain();
        }
      }
    }
  }
  if (TR) tr[2] = rt_clock();
  if (RES) residual_publish<NT>(r, partials, b);
  const double* sdt = block_dt_stage<NT>(dtl);
  if (neg) {
    atomicOr(&sc->neg_T, 1);
    if (OUT && !RES && !FX && P.host_sc) vm_drain();   // (done before host_mirror_tail's count)
  }
  __syncthreads();
  if (TR) tr[3] = rt_clock();
  if (threadIdx.x == 0) {
    block_dt_commit<NT>(sdt, sc, slot_next, serial, P.dt);
    if (TR) {
      vm_drain();
      tr[4] = rt_clock();
      unsigned long long* o = trace + (long)b * TILE_TRACE_WORDS;
#pragma unroll
      for (int q = 0; q < 5; q++) o[q] = tr[q];
      o[5] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID: wave/SIMD/CU/SE
      o[6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);   // XCC_ID
      o[7] = blockIdx.x;
    }
  }
  if (FX && threadIdx.x < WAVE && !(X.skip & 1)) fx_tail(X, sc, slot_next, seq_prev);
  if (!FX && !TR && (P.dt_fold || (OUT && !RES && P.host_sc)) && threadIdx.x < WAVE)
    host_mirror_tail(P, sc, slot_next);
}

// No occupancy attribute on the default kernel: the backend's own register
// budget (94 VGPRs here) beat every explicit amdgpu_waves_per_eu we tried.
template <bool RES, bool OUT, bool SG, int OCC = 0, int CPT = 1>
__global__ __launch_bounds__(BLOCK) void hf2d_lean_tile(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc,
                                                         int slot, int slot_next, int serial,
                                                         ResidualPack* partials, int part = 0) {
  lean_tile_body<RES, OUT, SG, CPT>(P, L, T, sc, slot, slot_next, serial, partials, FusedX{}, nullptr, part);
}

// Phase-traced plain step (profiling only, DeviceSolver::trace_tile).
template <bool SG, int CPT>
__global__ __launch_bounds__(BLOCK) void hf2d_lean_tile_tr(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc,
                                                            int slot, int slot_next, int serial,
                                                            ResidualPack* partials, unsigned long long* trace) {
  lean_tile_body<false, false, SG, CPT, false, true>(P, L, T, sc, slot, slot_next, serial, partials, FusedX{}, trace);
}

// Same step with the multi-GPU exchange fused in (FusedX).
template <bool RES, bool OUT, bool SG, int CPT>
// (the exchange arguments by pointer, read where they are used: by value
// they took ~26 SGPRs of the kernel arguments, and the 64-thread fused
// kernel spilled 96 SGPRs to VGPR lanes against 28 for the plain one)
__global__ __launch_bounds__(BLOCK) void hf2d_lean_tile_fx(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc,
                                                            int slot, int slot_next, int serial,
                                                            ResidualPack* partials, const FusedX* __restrict__ X) {
  lean_tile_body<RES, OUT, SG, CPT, true>(P, L, T, sc, slot, slot_next, serial, partials, *X);
}

// Small-strip geometries (single gas): NT = 128 / 64 threads per workgroup
// (picked by the ThreadBlockSize = 0 autotune per strip)
template <bool RES, bool OUT, int NT, int CPT>
__global__ __launch_bounds__(NT) void hf2d_lean_tile_nt(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc,
                                                       int slot, int slot_next, int serial, ResidualPack* partials,
                                                       int part = 0) {
  lean_tile_body<RES, OUT, true, CPT, false, false, NT>(P, L, T, sc, slot, slot_next, serial, partials, FusedX{},
                                                        nullptr, part);
}
template <bool RES, bool OUT, int NT, int CPT>
__global__ __launch_bounds__(NT) void hf2d_lean_tile_fx_nt(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc,
                                                          int slot, int slot_next, int serial,
                                                          ResidualPack* partials, const FusedX* __restrict__ X) {
  lean_tile_body<RES, OUT, true, CPT, true, false, NT>(P, L, T, sc, slot, slot_next, serial, partials, *X);
}
template <int NT, int CPT>
__global__ __launch_bounds__(NT) void hf2d_lean_tile_tr_nt(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc,
                                                          int slot, int slot_next, int serial,
                                                          ResidualPack* partials, unsigned long long* trace) {
  lean_tile_body<false, false, true, CPT, false, true, NT>(P, L, T, sc, slot, slot_next, serial, partials, FusedX{},
                                                           trace);
}
}  // namespace hf2d
