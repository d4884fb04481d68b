// Device-side helpers shared by the HIP translation units of the solver.
#pragma once

#include <hip/hip_runtime.h>

#include "../core/lean_euler.hpp"
#include "../core/stepkern.hpp"

namespace hf2d {

// Per-step scalars living on the device.
struct DevScalars {
  unsigned long long dt_bits[3];   // rotating dt slots (IEEE bits of positive doubles)
  double iter[3];                  // iteration number of the step using the slot
  double beta_min[3], cfl_min[3];  // scenario values of that iteration
  double time_part;                // accumulated dt since the cycle start
  int neg_T;
  int pad;
  double dt_val[3];                // dt of the step that used the slot (the lean
                                   // mechanism step's fill belongs to the previous one)
  unsigned hot_cnt[3];             // lean mechanism step: reacting cells listed by the step using the slot
  unsigned hot_cnt2[3];            // ... by its interior tiles (comm-overlap steps: a second list)
  // Lagged dt (StepParams::lag_dt): dt_lag[slot] is the dt of the step that
  // reads the slot -- the all-rank MIN of two steps back.  The first kernel
  // of step n (lag_head) moves MIN(slot n) -- the previous step's MIN, folded
  // over the ranks -- to dt_lag[slot of n + 1] before it overwrites the word.
  unsigned long long dt_lag[3];
  // Sharded dt MIN: every workgroup of a step used to atomicMin into ONE word,
  // and device-scope atomics to one address serialise at the memory side
  // (~10 ns each: the 800 workgroups of a small-strip step queued ~7 us
  // behind them).  Workgroup b min-reduces into shard
  // b % DT_SHARDS (one 128-byte line each) instead; the value of a slot is
  // MIN(dt_bits[slot], its shards) (dt_get), and folds that publish a
  // global MIN store it into dt_bits[slot] (the shards stay >= it).
  alignas(128) unsigned long long dt_sh[3][16][16];
};
constexpr int DT_SHARDS = 16;

__device__ inline double bits_to_d(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ inline unsigned long long d_to_bits(double d) { return (unsigned long long)__double_as_longlong(d); }

// Step n reads slot n%3, min-reduces into (n+1)%3 and resets (n+2)%3.
__host__ __device__ inline int slot_reset(int slot) { return (slot + 2) % 3; }

// (IEEE bits of positive doubles order like the values)
__host__ __device__ inline unsigned long long dt_bits_min(unsigned long long a, unsigned long long b) {
  return a < b ? a : b;
}
// value of a dt slot: the word and its shards (plain loads: the producers
// are earlier kernels)
__device__ inline double dt_get(const DevScalars* sc, int slot) {
  unsigned long long b = sc->dt_bits[slot];
#pragma unroll
  for (int k = 0; k < DT_SHARDS; k++) b = dt_bits_min(b, sc->dt_sh[slot][k][0]);
  return bits_to_d(b);
}
// same inside the producing kernel, after its workgroups' atomics (relaxed
// agent-scope loads)
__device__ inline double dt_get_fresh(DevScalars* sc, int slot) {
  unsigned long long b = __hip_atomic_load(&sc->dt_bits[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int k = 0; k < DT_SHARDS; k++)
    b = dt_bits_min(b, __hip_atomic_load(&sc->dt_sh[slot][k][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  return bits_to_d(b);
}
// a step's contribution (one thread per workgroup)
__device__ inline void dt_min(DevScalars* sc, int slot, double m) {
  atomicMin(&sc->dt_sh[slot][blockIdx.x % DT_SHARDS][0], d_to_bits(m));
}
__device__ inline void dt_reset(DevScalars* sc, int slot) {
  const unsigned long long one = d_to_bits(1.0);
  sc->dt_bits[slot] = one;
#pragma unroll
  for (int k = 0; k < DT_SHARDS; k++) sc->dt_sh[slot][k][0] = one;
}
__host__ inline unsigned long long dt_get_host(const DevScalars& s, int slot) {
  unsigned long long b = s.dt_bits[slot];
  for (int k = 0; k < DT_SHARDS; k++) b = dt_bits_min(b, s.dt_sh[slot][k][0]);
  return b;
}
__host__ inline void dt_set_host(DevScalars& s, int slot, unsigned long long b) {
  s.dt_bits[slot] = b;
  for (int k = 0; k < DT_SHARDS; k++) s.dt_sh[slot][k][0] = b;
}

// dt_get with one vector load per lane (lane k < DT_SHARDS: shard k, lane
// DT_SHARDS: the word) and a cross-lane MIN: the loads wait on vmcnt with the
// tile staging instead of on lgkmcnt with its LDS stores.  Every lane of the
// wavefront must be active.
__device__ inline double dt_get_wave(const DevScalars* sc, int slot) {
  const int lane = (int)(threadIdx.x & 63);
  unsigned long long b = ~0ull;
  if (lane < DT_SHARDS) b = sc->dt_sh[slot][lane][0];
  else if (lane == DT_SHARDS) b = sc->dt_bits[slot];
#pragma unroll
  for (int off = 1; off < 32; off <<= 1) b = dt_bits_min(b, (unsigned long long)__shfl_xor((long long)b, off, 64));
  return bits_to_d((unsigned long long)__shfl((long long)b, 0, 64));
}

// dt of the step reading the slot
__device__ inline double dt_cur(const StepParams& P, const DevScalars* sc, int slot) {
  return __builtin_expect(P.lag_dt != 0, 0) ? bits_to_d(sc->dt_lag[slot]) : dt_get(sc, slot);
}
// the lean tile kernel's read (StepParams::dt_read)
__device__ inline double dt_cur_tile(const StepParams& P, const DevScalars* sc, int slot) {
  if (__builtin_expect(P.lag_dt != 0, 0)) return bits_to_d(sc->dt_lag[slot]);
  if (P.dt_read == 2) return bits_to_d(sc->dt_bits[slot]);
  if (P.dt_read == 1) return dt_get_wave(sc, slot);
  return dt_get(sc, slot);
}
// first kernel of a lagged step, one thread (step_head), before the slot's
// word is overwritten with this step's dt: the previous step's MIN goes to the
// next step's lag word (fold: the MIN over the other ranks, if it is still
// pending)
__device__ inline void lag_head(const StepParams& P, DevScalars* sc, int slot, int slot_next, double fold = 1.0) {
  if (P.lag_dt) {
    const double m = dt_get(sc, slot);
    sc->dt_lag[slot_next] = d_to_bits(fold < m ? fold : m);
  }
}

__device__ inline void apply_dt(StepParams& P, const DevScalars* sc, int slot, bool tile = false) {
  const double dt = tile ? dt_cur_tile(P, sc, slot) : dt_cur(P, sc, slot);
  P.dt = dt;
  P.dtdx = dt / P.dx;
  P.dtdy = dt / P.dy;
  if (P.scen) {   // scenario values of this step's iteration (scenario_next)
    P.beta_min = sc->beta_min[slot];
    P.CFL_min = sc->cfl_min[slot];
  }
}

// apply_dt(tile) of the single-gas lean tile kernels in two parts, so that the
// dt read is in flight while the kernel issues its other loads: dt_tile_issue
// starts it (dt_read 1: this lane's word of dt_get_wave, not yet reduced;
// otherwise the slot's value), dt_tile_finish reduces it and sets P.dt and
// the two quotients.  Every lane of the wavefront must be active in both.
__device__ inline unsigned long long dt_tile_issue(StepParams& P, const DevScalars* sc, int slot) {
  if (P.scen) {   // scenario values of this step's iteration (scenario_next)
    P.beta_min = sc->beta_min[slot];
    P.CFL_min = sc->cfl_min[slot];
  }
  if (__builtin_expect(P.lag_dt != 0, 0)) return sc->dt_lag[slot];
  if (P.dt_read == 2) return sc->dt_bits[slot];
  if (P.dt_read == 1) {
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long b = ~0ull;
    if (lane < DT_SHARDS) b = sc->dt_sh[slot][lane][0];
    else if (lane == DT_SHARDS) b = sc->dt_bits[slot];
    return b;
  }
  return d_to_bits(dt_get(sc, slot));
}
__device__ inline void dt_tile_finish(StepParams& P, unsigned long long b) {
  if (!__builtin_expect(P.lag_dt != 0, 0) && P.dt_read == 1) {
#pragma unroll
    for (int off = 1; off < 32; off <<= 1) b = dt_bits_min(b, (unsigned long long)__shfl_xor((long long)b, off, 64));
    b = (unsigned long long)__shfl((long long)b, 0, 64);
  }
  const double dt = bits_to_d(b);
  P.dt = dt;
  P.dtdx = dt / P.dx;
  P.dtdy = dt / P.dy;
}

// Once per step (step_head): iteration number and CFL / beta scenario values
// (SolverBase::make_params arithmetic) of the next step.
__device__ inline void scenario_next(const StepParams& P, DevScalars* sc, int slot, int slot_next) {
  const double it = sc->iter[slot] + 1.0;
  sc->iter[slot_next] = it;
  if (P.scen) {
    const real bs = table_eval(P.scen->beta, it), cs = table_eval(P.scen->cfl, it);
    sc->beta_min[slot_next] = (bs < P.scen->beta0) ? bs : P.scen->beta0;   // std::min(beta0, bs)
    sc->cfl_min[slot_next] = (cs < P.scen->CFL) ? cs : P.scen->CFL;
  }
}

constexpr int BLOCK = 256;
constexpr int WAVE = 64;

// ---------------------------------------------------------------------------
// Wave-level residual reduction helpers
// ---------------------------------------------------------------------------
__device__ inline void shfl_merge(ResidualPack& r, int off) {
#pragma unroll
  for (int k = 0; k < NEQ; k++) {
    EqResidual o;
    o.dd_max = __shfl_xor(r.eq[k].dd_max, off, WAVE);
    o.i = __shfl_xor(r.eq[k].i, off, WAVE);
    o.j = __shfl_xor(r.eq[k].j, off, WAVE);
    o.rms = __shfl_xor(r.eq[k].rms, off, WAVE);
    o.sum_div = __shfl_xor(r.eq[k].sum_div, off, WAVE);
    o.count = __shfl_xor(r.eq[k].count, off, WAVE);
    EqResidual& f = r.eq[k];
    const bool later = (o.i > f.i) || (o.i == f.i && o.j > f.j);
    if (o.dd_max > f.dd_max || (o.dd_max == f.dd_max && later)) {
      f.dd_max = o.dd_max;
      f.i = o.i;
      f.j = o.j;
    }
    f.rms += o.rms;
    f.sum_div += o.sum_div;
    f.count += o.count;
  }
}

// A thread's residual before its cell, and the wave's merged pack into slot
// b * (NT / WAVE) + wave of the partials, by lane 0 (every lane active).
// Sites that write these and the helpers below out instead, because a kernel's
// registers or spills move with the call: profiles/step_epilogue_ab.md.
__device__ __forceinline__ void residual_begin(ResidualPack& r) {
  residual_reset(r);
#pragma unroll
  for (int k = 0; k < NEQ; k++) r.eq[k].i = r.eq[k].j = -1;
}
template <int NT>
__device__ __forceinline__ void residual_publish(ResidualPack& r, ResidualPack* partials, unsigned b) {
#pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) shfl_merge(r, off);
  if ((threadIdx.x & (WAVE - 1)) == 0) partials[(long)b * (NT / WAVE) + threadIdx.x / WAVE] = r;
}

// Once per step, by one thread of the step's first kernel (the caller tests
// for it), dt being the step's: resets the slot the NEXT step accumulates into
// (never the one this step min-reduces into, which other workgroups may
// already be writing), moves the lagged dt on, accumulates physical time and
// sets the next step's iteration and scenario values.  A kernel's own words
// (dt_val, hot_cnt, the host mirror) follow the call.  The three tile steps'
// heads keep the five lines written out: a change here goes there too.
__device__ __forceinline__ void step_head(const StepParams& P, DevScalars* sc, int slot, int slot_next, double dt,
                                          double fold = 1.0) {
  dt_reset(sc, slot_reset(slot));
  lag_head(P, sc, slot, slot_next, fold);
  sc->dt_bits[slot] = d_to_bits(dt);   // folded (later kernels of the step read the word)
  sc->time_part += dt;
  scenario_next(P, sc, slot, slot_next);
}

// MIN of a workgroup's dt limits into the slot the next step reads, around the
// caller's __syncthreads(): block_dt_stage, every thread: the wave's MIN into
// the workgroup's LDS words (returned); block_dt_commit, thread 0 after the
// barrier: their MIN into the slot's shard.  serial: the reference's serial
// build keeps dt a running minimum, so the step's dt joins in.  have_slot
// false sends nothing (the lean N-S materialize's fill: slot_next < 0);
// skip_unset sends nothing while the MIN is the initial 1.0 (hf2d_lnm_hot: a
// workgroup without a listed cell).  dtl and dt keep the caller's type, so the
// FP32 build converts where the written-out code did.
constexpr bool DT_HAVE_SLOT = true, DT_SKIP_UNSET = true;   // the guards, for a call that names them
template <int NT, class T>
__device__ __forceinline__ double* block_dt_stage(T dtl) {
  __shared__ double sdt[NT / WAVE];
  for (int off = 1; off < WAVE; off <<= 1) dtl = fmin(dtl, __shfl_xor(dtl, off, WAVE));
  if ((threadIdx.x & (WAVE - 1)) == 0) sdt[threadIdx.x / WAVE] = dtl;
  return sdt;
}
template <int NT, class T>
__device__ __forceinline__ void block_dt_commit(const double* sdt, DevScalars* sc, int slot_next, int serial, T dt,
                                                bool have_slot = true, bool skip_unset = false) {
  double m = sdt[0];
  for (int q = 1; q < NT / WAVE; q++) m = fmin(m, sdt[q]);
  if (serial) m = fmin(m, dt);
  if (have_slot && (!skip_unset || m < 1.0)) dt_min(sc, slot_next, m);
}

// Cell (i, j) of the flat x-major index c of the one-cell-per-thread kernels.
struct CellIJ {
  int i, j;
};
__device__ __forceinline__ CellIJ cell_ij(long c, int ny) {
  const int i = (int)(c / ny);
  return {i, (int)(c - (long)i * ny)};
}

// Workgroups are dispatched round-robin over the 8 XCDs (each with its own
// L2).  Remap so XCD x owns a contiguous run of tiles: the i+-1 neighbour
// columns a tile reads then sit in the same L2.  Bijective on [0, n).
constexpr unsigned NUM_XCD = 8;
__device__ inline unsigned xcd_remap(unsigned b, unsigned n) {
  const unsigned q = n / NUM_XCD;
  if (b >= q * NUM_XCD) return b;
  return (b % NUM_XCD) * q + b / NUM_XCD;
}

// ---------------------------------------------------------------------------
// Multi-GPU exchange pieces the kernel families share (no __global__ here):
//   ColList, FusedX        halo field list / mailbox arguments of a fused exchange
//   p2p_*, fx_*            system-scope mailbox loads and stores, peer waits, the fused tail,
//                          the ghost prologue and edge push of the fused lean N-S / mechanism steps
//   tile_of_part, tile_edge_first   workgroup -> tile orders of the edge-first launches
// ---------------------------------------------------------------------------
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

// Every bit of v stays live up to this point.  For the destination of a load
// still in flight of which the code uses only a part: the register allocator
// otherwise hands the unused half to a new value right away, and the write
// to it has to wait for the load (s_waitcnt) in front of whatever was meant
// to be issued behind it.  Place it where the load is waited for anyway.
__device__ inline void keep_whole(u64& v) { asm volatile("" : "+v"(v)); }

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

constexpr int LNS_SKIP_ERR = 8;   // neg_T bit: fill_node() skipped a node (rho == 0 or k < 1)

// Ghost prologue of a fused lean N-S / mechanism step (replaces the separate
// hf2d_p2p_unpack launch after the previous fused step): a tile whose fills
// read a ghost column copies the rows it reads, [j0 - 1, j0 + TJ], of every
// HALO_LNS entry of the previous step's list Lg from this rank's mailbox of
// parity seq_prev (the previous kernel's tail acquired the peers' flags) into
// the ghost columns; the workgroup barrier makes them visible to its own
// loads.  Vertically adjacent edge tiles write the rows they share with the
// same values, and every ghost value a tile reads it wrote itself: a
// workgroup reads its own stores through its CU's L1 (workgroup-scope
// coherence needs no cache maintenance outside thread-group-split mode; an
// agent-scope acquire here invalidates the XCD's L2 lines and measured
// 14.8 -> 23.3 us of exchange cost on the 4-rank Step strip).
__device__ inline void fx_ghost_prologue(const StepParams& P, const FusedX& X, const ColList* Lg, int i0, int j0,
                                         int TI, int TJ, unsigned long long seq_prev) {
  const bool gl = (X.sides & 1) && i0 <= P.i0 + 1;
  const bool gr = (X.sides & 2) && i0 + TI + 1 >= P.i1;
  if (!gl && !gr) return;
  const int par = (int)(seq_prev & 1), nf = Lg->nf;
  const int jlo = j0 > 0 ? j0 - 1 : 0, jhi = j0 + TJ + 1 < P.ny ? j0 + TJ + 1 : P.ny;
  const int rows = jhi - jlo, per_side = nf * rows;
  for (int t = (int)threadIdx.x; t < 2 * per_side; t += (int)blockDim.x) {
    const int side = t < per_side ? 0 : 1;
    if (side == 0 ? !gl : !gr) continue;
    const int tt = t - side * per_side, f = tt / rows, j = jlo + (tt - f * rows);
    const real v = p2p_load(X.my_recv + ((long)par * 2 + side) * X.cap + (long)f * P.ny + j);
    Lg->f[f][(long)(side == 0 ? P.i0 - 1 - Lg->o[f] : P.i1 + Lg->o[f]) * P.ny + j] = v;
  }
  __syncthreads();
}

// Edge push of a fused lean N-S step, by every thread of an edge tile after
// the tile's barrier: the HALO_LNS values of the tile's cells in the strip's
// first / last two columns (entry f of Lc at column P.i0 + o[f] / P.i1 - 1 -
// o[f], stored by their owner threads before the barrier) -> the neighbour's
// mailbox of parity seq_prev + 1, K independent loads then K stores per
// thread; drained, then a barrier, so the tail counts a workgroup whose
// mailbox stores have completed.  (The owner threads pushing their own
// cells -- one column of 20 threads per offset, ~20 fields each -- kept the
// edge tiles, the last to finish in a one-round grid, ~4.6 us longer on the
// resonator's 4-rank strip, tools/exchange_loopback.py.)
__device__ inline void fx_edge_push(const StepParams& P, const FusedX& X, const ColList* Lc, const LeanTile& T, int i0,
                                    int j0, unsigned long long seq_prev) {
  const bool el = (X.sides & 1) && i0 <= P.i0 + 1;
  const bool er = (X.sides & 2) && i0 + T.TI >= P.i1 - 1;
  if (!el && !er) return;   // (uniform over the workgroup)
  const int pn = (int)((seq_prev + 1) & 1);
  const int jhi = j0 + T.TJ < P.ny ? j0 + T.TJ : P.ny, rows = jhi - j0, nf = Lc->nf;
  const int per = nf * rows, total = (el && er ? 2 : 1) * per;
  constexpr int K = 4;
  for (int base = (int)threadIdx.x; base < total; base += K * BLOCK) {
    real v[K];
    real* dst[K];
#pragma unroll
    for (int u = 0; u < K; u++) {
      const int t = base + u * BLOCK;
      dst[u] = nullptr;
      v[u] = 0.0;
      if (t < total) {
        const int side = (el && er) ? t / per : (el ? 0 : 1);
        const int tt = (el && er) ? t - side * per : t, f = tt / rows, j = j0 + (tt - f * rows), o = Lc->o[f];
        const int col = side == 0 ? P.i0 + o : P.i1 - 1 - o;
        if (col >= i0 && col < i0 + T.TI && col >= P.i0 && col < P.i1) {
          dst[u] = (side == 0 ? X.peer_recv_l + ((long)pn * 2 + 1) * X.cap : X.peer_recv_r + ((long)pn * 2) * X.cap) +
                   (long)f * P.ny + j;
          v[u] = Lc->f[f][(long)col * P.ny + j];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < K; u++)
      if (dst[u]) p2p_store(dst[u], v[u]);
  }
  vm_drain();
  __syncthreads();
}

}  // namespace hf2d
