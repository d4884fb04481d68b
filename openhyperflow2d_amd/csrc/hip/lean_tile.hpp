// Inviscid lean tile kernels (lean_euler.hpp on LDS tiles) and what their
// fused multi-GPU exchange shares with the halo kernels (halo_kernels.hpp):
//   ColList, FusedX        halo field list / mailbox arguments of a fused exchange
//   p2p_*, fx_*            system-scope mailbox loads and stores, peer waits, the fused tail
//   lean_tile_body         the tile step; hf2d_lean_tile and its _fx (fused
//                          exchange), _tr (phase trace), _nt (128 / 64 threads)
//                          and _occ (register budget) forms
// Part of the device_solver.hip translation unit.
#pragma once

#include "../core/lean_euler.hpp"
#include "dev_common.hpp"

namespace hf2d {

// Halo pack: nf field columns (each ny contiguous doubles at src[f] + col*ny)
constexpr int MAX_HALO_FIELDS = 128;   // 4*NEQ + 5 state fields + up to 16 species x 4
// Halo field list: entry f is column (first + o[f]) / (last - o[f]) of
// field f on the sending side and ghost column (ghostL - o[f]) / (ghostR +
// o[f]) on the receiving side: o = 1 carries the second column of a
// two-column halo (the lean N-S / mechanism kernels on strips).
struct ColList {
  real* f[MAX_HALO_FIELDS];
  unsigned char o[MAX_HALO_FIELDS] = {};
  int nf;
};
constexpr long P2P_SPIN_LIMIT = 1L << 26;   // ~3 s of s_sleep polling, then give up (neg_T bit 2)
constexpr int P2P_THREADS = 512;

// Acquire load of a peer's publication flag at system scope: the poll loops
// spin with relaxed loads (cheap) and finish with this one, so every later
// load (mailbox data, peer dt) is ordered after the observed flag.
__device__ inline unsigned long long p2p_acquire(const unsigned long long* f) {
  return __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ inline double p2p_load(const double* p) {
  return __longlong_as_double((long long)__hip_atomic_load((const unsigned long long*)p, __ATOMIC_RELAXED,
                                                           __HIP_MEMORY_SCOPE_SYSTEM));
}
// (FP32 build: the halo values are floats; the dt words stay doubles)
__device__ inline float p2p_load(const float* p) {
  return __int_as_float((int)__hip_atomic_load((const unsigned*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}

// Multi-GPU exchange fused into the lean tile kernel (xGMI mailboxes, see
// hf2d_p2p_xchg for the layout and the parity argument).  Step s of a rank:
//   start  the dt slot already holds the global MIN (folded by the previous
//          kernel's last workgroup); tiles at the strip edges stage their
//          ghost column straight from the mailbox of parity s-1;
//   end    cells of the first / last owned column store their new lean
//          state into the neighbour's mailbox of parity s with
//          system-coherent stores and wait for their completion (vmcnt);
//          the last workgroup to finish (completion counter) sends this
//          rank's local dt MIN to every peer, publishes flag s, waits
//          (bounded) for the peers' flag s and folds their dt into the slot.
// One kernel per step and a single waiting workgroup, at the tail: no
// exchange kernel, no pack/unpack pass, no host involvement, and no
// system-scope fence (L2 writeback / invalidate) in the other workgroups.
// Ghost columns of the state arrays are only refreshed by
// hf2d_p2p_complete, which the host runs before any other consumer.
__device__ inline void p2p_store(double* p, double v) {
  __hip_atomic_store((unsigned long long*)p, (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ inline void p2p_store(float* p, float v) {
  __hip_atomic_store((unsigned*)p, (unsigned)__float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
// outstanding vector-memory operations of this wave (stores included on gfx9)
// have completed: the ordering point for the relaxed system-coherent stores
__device__ inline void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ inline unsigned long long rt_clock() { return __builtin_amdgcn_s_memrealtime(); }
constexpr int FX_DONE_STRIDE = 32;   // completion counters on lines of their own
// tail phase trace (HF2D_FX_SKIP bit 4, loopback timing runs only): after the
// counters, FX_TRACE_N records of FX_TRACE_W clocks, one per step (seq mod N)
constexpr int FX_TRACE_N = 64, FX_TRACE_W = 8;
constexpr unsigned FX_COUNT1_MAX = 512;
constexpr int FX_DONE_WORDS = (DT_SHARDS + 1) * FX_DONE_STRIDE + 2 * FX_TRACE_N * FX_TRACE_W;
struct FusedX {
  real* peer_recv_l;   // left neighbour's mailbox recv base (we are its right side)
  real* peer_recv_r;
  const real* my_recv;
  unsigned long long* const* peer_flags;
  double* const* peer_dtr;
  const unsigned long long* my_flags;
  const double* my_dtr;
  unsigned long long* seq;   // last published sequence number
  unsigned* done;            // workgroups finished in this step: per dt shard, then the shards (FX_DONE_STRIDE apart)
  long cap;
  int rank, nranks, sides, on;
  // lagged dt: the tail waits for the two neighbours' flags only and leaves
  // the dt MIN to the next step's first workgroup (lean_tile_body) or to
  // hf2d_p2p_complete
  int defer;
  // cost attribution of the fused exchange (HF2D_FX_SKIP, timing only, wrong
  // results): bit 0 no tail, bit 1 no edge pushes / mailbox stores, bit 2
  // ghosts staged from the state arrays instead of the mailbox (no ghost
  // prologue), bit 3 no loads of the push kernel
  int skip;
  int edge_first;   // inviscid fused tile kernel: edge tile columns dispatched first (HF2D_FX_EDGE_FIRST)
  // tail completion count: one per dt shard + one for the shards, or one
  // counter where the caller asks for it (fused lean N-S kernel, grids of <=
  // FX_COUNT1_MAX workgroups); HF2D_FX_COUNT1 = 1 / 2 forces one / two levels.
  // Loopback tail trace: the resonator's 4-rank strip (420 workgroups that
  // finish spread out) 0.96 -> 0.52 us of counting and 4.4 -> 3.4 us of
  // exchange with one counter; workgroups that finish together contend on it:
  // the headline's 8-rank strip (719 single-wave workgroups) 5.5 -> 11.7 us,
  // the scramjet's push kernel (135) 1.5 - 1.7 us of counting
  int count1;
};

// Peer waits and publications are spread over the lanes of one wavefront:
// lane q polls / publishes to peer q (q < nranks <= 64 per pass), so a step
// costs one round trip to the fine-grained mailbox per phase instead of one
// per peer (the single-thread loops cost ~12 us per step on an 8-rank strip,
// tools/exchange_loopback.py, profiles/exchange_loopback_r05.md).
__device__ inline double wave_min(double v) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) v = fmin(v, __shfl_xor(v, off, WAVE));
  return v;
}
// Every lane of the calling wavefront: wait (bounded) for the flags of the
// peers q with need(q) to reach target (acquire), and return the MIN of
// their dt of parity par (fold) -- or 1.0 without fold.  False through *ok
// after a timeout (neg_T bit 2) or an earlier one.
template <class Need>
__device__ inline double p2p_wait_wave(const FusedX& x, unsigned long long target, DevScalars* sc, Need need,
                                       bool fold, int par, bool* ok) {
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  bool good = !(__hip_atomic_load(&sc->neg_T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2);
  double d = 1.0;
  for (int q = lane; q < x.nranks && good; q += WAVE) {
    if (q == x.rank || !need(q)) continue;
    long spins = 0;
    while (__hip_atomic_load(&x.my_flags[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < target) {
      __builtin_amdgcn_s_sleep(1);
      if (++spins > P2P_SPIN_LIMIT) {
        atomicOr(&sc->neg_T, 2);
        good = false;
        break;
      }
    }
    // acquire the peer's publication: its dt and mailbox stores (released by
    // its vmcnt drain before the flag) are visible to every load ordered
    // after this one, here and in later kernels
    if (good) (void)p2p_acquire(&x.my_flags[q]);
    if (good && fold) d = fmin(d, p2p_load(x.my_dtr + par * x.nranks + q));
  }
  *ok = __ballot(!good) == 0;
  return wave_min(d);
}
__device__ inline bool p2p_wait_all(const FusedX& x, unsigned long long target, DevScalars* sc) {
  bool ok;
  (void)p2p_wait_wave(x, target, sc, [](int) { return true; }, false, 0, &ok);
  return ok;
}

// Tail of a step kernel with the exchange fused in (wavefront 0 of every
// workgroup, after the workgroup's mailbox stores and dt MIN): the last
// workgroup to finish publishes this rank's step (its dt to every peer, then
// flag seq_prev + 1), waits (bounded) for every peer's flag of the same step
// -- the two neighbours' only with X.defer -- and folds their dt into the
// slot the next step reads.
// Returns true (every lane) in the last workgroup, after the wait.
__device__ __forceinline__ bool fx_tail(const FusedX& X, DevScalars* sc, int slot_next,
                                        unsigned long long seq_prev, bool fold = true, bool one_level = false) {
  const int lane = (int)(threadIdx.x & (WAVE - 1));
  const bool trace = (X.skip & 16) != 0;
  unsigned long long c[FX_TRACE_W] = {};
  if (trace) c[0] = rt_clock();
  // the workgroup barrier drained every wave's mailbox stores; drain lane
  // 0's dt atomic before counting this workgroup as done
  vm_drain();
  if (trace) c[1] = rt_clock();
  // completion count in two levels (one counter per dt shard, then one for
  // the shards): a single counter serialises every workgroup's returning
  // atomic at the memory side
  int last = 0;
  if (lane == 0 && (X.count1 == 1 || (X.count1 == 0 && one_level))) {
    unsigned* ct = X.done + DT_SHARDS * FX_DONE_STRIDE;
    if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1) {
      __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last = 1;
    }
  } else if (lane == 0) {
    const unsigned G = gridDim.x, sh = blockIdx.x % DT_SHARDS;
    const unsigned pop = (G - sh + DT_SHARDS - 1) / DT_SHARDS, nsh = G < DT_SHARDS ? G : DT_SHARDS;
    unsigned* cs = X.done + sh * FX_DONE_STRIDE;
    unsigned* ct = X.done + DT_SHARDS * FX_DONE_STRIDE;
    if (__hip_atomic_fetch_add(cs, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == pop - 1) {
      __hip_atomic_store(cs, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_fetch_add(ct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nsh - 1) {
        __hip_atomic_store(ct, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = 1;
      }
    }
  }
  if (!__shfl(last, 0, WAVE)) return false;
  if (trace) c[2] = rt_clock();
  // last workgroup: this rank's dt (word + shards, one per lane), published
  // to every peer (one peer per lane), then the flags, then the peers'
  const unsigned long long sn = seq_prev + 1;
  const int pn = (int)(sn & 1);
  unsigned long long b = ~0ull;
  if (lane < DT_SHARDS)
    b = __hip_atomic_load(&sc->dt_sh[slot_next][lane][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (lane == DT_SHARDS) b = __hip_atomic_load(&sc->dt_bits[slot_next], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  double d = wave_min(b == ~0ull ? 1.0 : bits_to_d(b));
  if (trace) c[3] = rt_clock();
  for (int q = lane; q < X.nranks; q += WAVE)
    if (q != X.rank) p2p_store(X.peer_dtr[q] + pn * X.nranks + X.rank, d);
  vm_drain();   // (the wavefront's stores: every lane's)
  if (trace) c[4] = rt_clock();
  for (int q = lane; q < X.nranks; q += WAVE)
    if (q != X.rank) __hip_atomic_store(&X.peer_flags[q][X.rank], sn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (trace) c[5] = rt_clock();
  const bool defer = X.defer != 0;
  const int r = X.rank;
  bool ok;
  const double peers = p2p_wait_wave(X, sn, sc, [=](int q) { return !defer || q == r - 1 || q == r + 1; },
                                     fold && !defer, pn, &ok);
  d = fmin(d, peers);
  if (trace) c[6] = rt_clock();
  if (lane == 0) {
    if (fold && !defer && ok)
      __hip_atomic_store(&sc->dt_bits[slot_next], d_to_bits(d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *X.seq = sn;
    if (trace) {
      vm_drain();
      c[7] = rt_clock();
      unsigned long long* o = reinterpret_cast<unsigned long long*>(X.done + (DT_SHARDS + 1) * FX_DONE_STRIDE) +
                              (long)(sn % FX_TRACE_N) * FX_TRACE_W;
#pragma unroll
      for (int k = 0; k < FX_TRACE_W; k++) o[k] = c[k];
    }
  }
  return true;
}


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

// part: 0 every tile; 1 the tiles of the strip's first and last tile column
// (their results feed the halo exchange); 2 the other tiles.  The grid of a
// part launch has exactly that many workgroups (DeviceSolver comm overlap).
__device__ inline unsigned tile_of_part(unsigned bl, int part, const LeanTile& T) {
  if (part == 1) return bl < (unsigned)T.nbj ? bl : (unsigned)((T.nbi - T.ne) * T.nbj) + (bl - T.nbj);
  if (part == 2) return (unsigned)T.nbj + bl;
  return bl;
}

// all tiles, the strip's edge tile columns first (the first one, then the
// last T.ne), then the interior ones in order
__device__ inline unsigned tile_edge_first(unsigned bl, const LeanTile& T) {
  const unsigned nbj = (unsigned)T.nbj, ne = (unsigned)T.ne, nbi = (unsigned)T.nbi;
  if (nbi < 2 + ne || bl < nbj) return bl;
  if (bl < (1 + ne) * nbj) return (nbi - ne) * nbj + (bl - nbj);
  return nbj + (bl - (1 + ne) * nbj);
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
  apply_dt(P, sc, slot, true);
  if (b == 0 && threadIdx.x < WAVE) {
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
      if (OUT && !RES && !FX && P.host_sc) host_mirror_head(P, sc, slot_next);
    }
  }
  int i[CPT], j[CPT], c[CPT], i0, j0;
  bool mine[CPT];
  // own-cell global inputs first, so they are in flight during the staging
  LeanOwn own[CPT];
#pragma unroll
  for (int q = 0; q < CPT; q++) {
    mine[q] = lean_tile_cell(P, T, (int)b, (int)threadIdx.x, &i[q], &j[q], &c[q], &i0, &j0, q);
    if (mine[q]) lean_load_own<TileIO<SG>::NE>(L, (long)i[q] * P.ny + j[q], own[q]);
  }
  if (!FX || seq_prev == 0 || (X.skip & 4) || (i0 - 1 > P.i0 - 1 && i0 + T.TI < P.i1)) {
    lean_tile_stage<SG>(P, L, T, i0, j0, lds, threadIdx.x, NT);
  } else {
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
  __syncthreads();
  // (raising the wave priority here for the compute phase, s_setprio 2,
  // measured no change: headline 26.9 - 27.2 us either way, triple point
  // 350 - 353 us)
  if (TR) tr[1] = rt_clock();
  ResidualPack r;
  if (RES) {
    residual_reset(r);
#pragma unroll
    for (int k = 0; k < NEQ; k++) r.eq[k].i = r.eq[k].j = -1;
  }
  double dtl = 1.0;
  int neg = 0;
#pragma unroll
  for (int q = 0; q < CPT; q++) {
    if (mine[q]) {
      TileIO<SG> io(L, (long)i[q] * P.ny + j[q], lds, T.NC, T.W, c[q]);
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
  if (RES) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) shfl_merge(r, off);
    if ((threadIdx.x & (WAVE - 1)) == 0) partials[(long)b * (NT / WAVE) + threadIdx.x / WAVE] = r;
  }
  for (int off = 1; off < WAVE; off <<= 1) dtl = fmin(dtl, __shfl_xor(dtl, off, WAVE));
  __shared__ double sdt[NT / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) sdt[threadIdx.x / WAVE] = dtl;
  if (neg) {
    atomicOr(&sc->neg_T, 1);
    if (OUT && !RES && !FX && P.host_sc) vm_drain();   // (done before host_mirror_tail's count)
  }
  __syncthreads();
  if (TR) tr[3] = rt_clock();
  if (threadIdx.x == 0) {
    double m = sdt[0];
    for (int q = 1; q < NT / WAVE; q++) m = fmin(m, sdt[q]);
    if (serial) m = fmin(m, P.dt);
    dt_min(sc, slot_next, m);
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

template <bool RES, bool OUT, bool SG, int OCC, int CPT = 1>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(OCC)))
void hf2d_lean_tile_occ(StepParams P, LeanSoA L, LeanTile T, DevScalars* sc, int slot, int slot_next, int serial,
                        ResidualPack* partials) {
  lean_tile_body<RES, OUT, SG, CPT>(P, L, T, sc, slot, slot_next, serial, partials);
}
}  // namespace hf2d
