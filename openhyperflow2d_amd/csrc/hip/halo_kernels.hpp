// Halo and mailbox kernels of the strip decomposition:
//   hf2d_pack/unpack(2)    halo columns to / from the send and receive buffers (RCCL, in-process group)
//   hf2d_dt_commit/fold_dt the dt MIN of the host transports
//   hf2d_p2p_xchg          xGMI mailbox exchange in one workgroup (P2PArgs)
//   hf2d_p2p_complete      ghost columns + dt after fused tile steps
//   hf2d_p2p_push/finish/unpack   multi-workgroup mailbox exchange
// Included by transport.hip only (the kernels here are not templates).
#pragma once

#include "dev_common.hpp"

namespace hf2d {

__global__ void hf2d_pack(ColList L, int col, int ny, real* buf) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L.nf * ny) return;
  const int f = t / ny, j = t - f * ny;
  buf[t] = L.f[f][(long)col * ny + j];
}
__global__ void hf2d_unpack(ColList L, int col, int ny, const real* buf) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= L.nf * ny) return;
  const int f = t / ny, j = t - f * ny;
  L.f[f][(long)col * ny + j] = buf[t];
}
// Both sides in one launch (sides: bit 0 left, bit 1 right).
// dt slot's shards into its word (before a host transport sends the word)
__global__ void hf2d_dt_commit(DevScalars* sc, int slot) {
  if (threadIdx.x == 0) sc->dt_bits[slot] = d_to_bits(dt_get(sc, slot));
}
// MIN of the peers' dt into this rank's slot (exchange_dt, in-process group)
__global__ void hf2d_fold_dt(DevScalars* sc, int slot, const double* dt_recv, int nranks, int rank) {
  if (threadIdx.x != 0) return;
  double m = dt_get(sc, slot);
  for (int q = 0; q < nranks; q++)
    if (q != rank) m = fmin(m, dt_recv[q]);
  sc->dt_bits[slot] = d_to_bits(m);
}

// (dslot >= 0: also commits that dt slot's shards into its word, which the
// host transports send)
__global__ void hf2d_pack2(ColList L, int colL, int colR, int ny, real* bufL, real* bufR, int sides,
                           DevScalars* sc, int dslot) {
  const int cnt = L.nf * ny;
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && dslot >= 0) sc->dt_bits[dslot] = d_to_bits(dt_get(sc, dslot));
  const bool right = t >= cnt;
  if (right) t -= cnt;
  if (t >= cnt || !(sides & (right ? 2 : 1))) return;
  const int f = t / ny, j = t - f * ny;
  (right ? bufR : bufL)[t] = L.f[f][(long)(right ? colR - L.o[f] : colL + L.o[f]) * ny + j];
}
// Also folds the dt gathered from the other ranks (ndt > 0: dtr[q], q != self)
// into the next dt slot: MIN of positive doubles, exact in any order.
__global__ void hf2d_unpack2(ColList L, int colL, int colR, int ny, const real* bufL, const real* bufR,
                             int sides, DevScalars* sc, int dslot, const double* dtr, int ndt, int self) {
  const int cnt = L.nf * ny;
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0 && ndt > 0) {
    double m = dt_get(sc, dslot);
    for (int q = 0; q < ndt; q++)
      if (q != self) m = fmin(m, dtr[q]);
    sc->dt_bits[dslot] = d_to_bits(m);
  }
  const bool right = t >= cnt;
  if (right) t -= cnt;
  if (t >= cnt || !(sides & (right ? 2 : 1))) return;
  const int f = t / ny, j = t - f * ny;
  L.f[f][(long)(right ? colR + L.o[f] : colL - L.o[f]) * ny + j] = (right ? bufR : bufL)[t];
}

// ---------------------------------------------------------------------------
// xGMI peer-to-peer halo transport (default for multi-GPU strips).
//
// Every rank owns one fine-grained "mailbox" allocation, mapped into its
// peers with IPC handles:
//   flags[nranks]  u64   step sequence number last published by rank q
//   dtr[2][nranks] f64   dt of rank q for sequence parity 0/1
//   recv[2][2][cap] f64  halo columns for parity 0/1 from the left/right
// One single-workgroup kernel per exchange replaces pack + RCCL group +
// unpack: it stores this rank's boundary columns straight into the
// neighbours' mailboxes and its dt into every peer's, publishes its flag,
// waits (bounded) for every peer's flag of the same sequence number, then
// unpacks its own mailbox into the ghost columns and folds the MIN of all dt
// into the next dt slot -- bitwise the RCCL path's result.
// Ordering without system-scope fences: mailbox data and flags are written
// with system-coherent stores (p2p_store: they bypass the non-coherent L2),
// and a wave's stores are complete (s_waitcnt vmcnt(0)) before any flag is
// stored; a reader issues its system-coherent data loads only after it has
// seen the flag.  A __threadfence_system() would also write back the whole
// L2 of the XCD (buffer_wbl2), which cost ~3 us per step in the fused kernel.
// Parity double buffering is safe without a second handshake: a peer writes
// parity p again only at sequence s+2, after it has seen this rank's flag
// s+1, which is published after the unpack of s.  The sequence counter lives
// in device memory, so the kernel replays unchanged inside step graphs.
// ---------------------------------------------------------------------------


struct P2PArgs {
  ColList L;
  int first, last, ghostL, ghostR, ny, cnt, sides;
  long cap;                              // doubles per (parity, side) mailbox slot
  real* peer_recv_l;                     // left neighbour's recv base (this rank is its right side)
  real* peer_recv_r;                     // right neighbour's recv base
  real* my_recv;
  unsigned long long* const* peer_flags; // [nranks] flag array of each rank (self: own)
  double* const* peer_dtr;               // [nranks] dtr array of each rank
  unsigned long long* my_flags;
  double* my_dtr;
  unsigned long long* seq;               // device-side sequence counter
  DevScalars* sc;
  int dslot, fold_dt, rank, nranks;
};



__global__ __launch_bounds__(P2P_THREADS) void hf2d_p2p_xchg(P2PArgs a) {
  const unsigned long long seq = *a.seq + 1;
  const int par = (int)(seq & 1);
  const int ny = a.ny;
  // 1. push boundary columns and this rank's dt into the peers' mailboxes:
  // PER loads of a thread in flight, then its PER system-coherent stores (one
  // load latency per batch instead of one per value: the N-S halo is 23-43
  // fields x ny per side)
  constexpr int PER = 16;
  const int total = ((a.sides & 1) ? a.cnt : 0) + ((a.sides & 2) ? a.cnt : 0);
  for (int base = 0; base < total; base += PER * P2P_THREADS) {
    real v[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
      const int t = base + u * P2P_THREADS + threadIdx.x;
      if (t < total) {
        const bool right = !(a.sides & 1) || t >= a.cnt;
        const int tt = (a.sides & 1) && right ? t - a.cnt : t;
        const int f = tt / ny, j = tt - f * ny;
        v[u] = a.L.f[f][(long)(right ? a.last - a.L.o[f] : a.first + a.L.o[f]) * ny + j];
      }
    }
#pragma unroll
    for (int u = 0; u < PER; u++) {
      const int t = base + u * P2P_THREADS + threadIdx.x;
      if (t < total) {
        const bool right = !(a.sides & 1) || t >= a.cnt;
        const int tt = (a.sides & 1) && right ? t - a.cnt : t;
        // the left neighbour receives "from right", the right one "from left"
        real* dst = right ? a.peer_recv_r + ((long)par * 2) * a.cap : a.peer_recv_l + ((long)par * 2 + 1) * a.cap;
        p2p_store(dst + tt, v[u]);
      }
    }
  }
  const double mydt = dt_get(a.sc, a.dslot);
  for (int q = threadIdx.x; q < a.nranks; q += P2P_THREADS)
    if (q != a.rank) p2p_store(a.peer_dtr[q] + par * a.nranks + a.rank, mydt);
  // system-coherent stores drained (vmcnt) in every wave before the flag:
  // no L2 writeback needed, nothing of this kernel sits dirty in the L2
  vm_drain();
  __syncthreads();
  // 2. publish, 3. wait for every peer's publication of the same sequence
  for (int q = threadIdx.x; q < a.nranks; q += P2P_THREADS)
    if (q != a.rank) __hip_atomic_store(&a.peer_flags[q][a.rank], seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const bool failed = __hip_atomic_load(&a.sc->neg_T, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 2;
  __shared__ double s_dt[P2P_THREADS];
  double dmin = mydt;   // each polling thread folds the dt of the peers it waited for
  for (int q = threadIdx.x; q < a.nranks; q += P2P_THREADS) {
    if (q == a.rank || failed) continue;   // after one timeout, stop waiting (the host reports it)
    long spins = 0;
    bool ok = true;
    while (__hip_atomic_load(&a.my_flags[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) < seq) {
      __builtin_amdgcn_s_sleep(2);
      if (++spins > P2P_SPIN_LIMIT) {
        atomicOr(&a.sc->neg_T, 2);
        ok = false;
        break;
      }
    }
    if (ok) (void)p2p_acquire(&a.my_flags[q]);   // order the mailbox reads after the flag
    if (ok) dmin = fmin(dmin, p2p_load(a.my_dtr + par * a.nranks + q));
  }
  s_dt[threadIdx.x] = dmin;
  __syncthreads();
  // 4. unpack this rank's mailbox into the ghost columns: all loads of a
  // thread first, then its stores (the stores may alias nothing the loads
  // read, but the compiler cannot know that)
  for (int base = 0; base < total; base += PER * P2P_THREADS) {
    real v[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
      const int t = base + u * P2P_THREADS + threadIdx.x;
      if (t < total) {
        const bool right = !(a.sides & 1) || t >= a.cnt;
        const int tt = (a.sides & 1) && right ? t - a.cnt : t;
        v[u] = p2p_load(a.my_recv + ((long)par * 2 + (right ? 1 : 0)) * a.cap + tt);
      }
    }
#pragma unroll
    for (int u = 0; u < PER; u++) {
      const int t = base + u * P2P_THREADS + threadIdx.x;
      if (t < total) {
        const bool right = !(a.sides & 1) || t >= a.cnt;
        const int tt = (a.sides & 1) && right ? t - a.cnt : t;
        const int f = tt / ny, j = tt - f * ny;
        a.L.f[f][(long)(right ? a.ghostR + a.L.o[f] : a.ghostL - a.L.o[f]) * ny + j] = v[u];
      }
    }
  }
  // 5. global dt: MIN over ranks (exact in any order)
  if (threadIdx.x == 0) {
    if (a.fold_dt) {
      double m = mydt;
      for (int q = 0; q < a.nranks && q < P2P_THREADS; q++) m = fmin(m, s_dt[q]);
      a.sc->dt_bits[a.dslot] = d_to_bits(m);
    }
    *a.seq = seq;
  }
}

// Ghost columns + global dt after fused steps, for any other consumer: wait
// for the peers' last publication, copy the mailbox of that parity into the
// ghost columns of the current state, fold the dt MIN into the slot.
__global__ __launch_bounds__(P2P_THREADS) void hf2d_p2p_complete(ColList Lc, int ghostL, int ghostR, int ny, int cnt,
                                                                 FusedX X, DevScalars* sc, int dslot) {
  const unsigned long long sq = *X.seq;
  if (sq == 0) return;
  __shared__ int ok;
  if (threadIdx.x < WAVE) {
    const bool w = p2p_wait_all(X, sq, sc);
    if (threadIdx.x == 0) ok = w ? 1 : 0;
  }
  __syncthreads();
  if (!ok) return;
  const int pp = (int)(sq & 1);
  if (X.sides & 1) {
    const real* src = X.my_recv + ((long)pp * 2) * X.cap;
    for (int t = threadIdx.x; t < cnt; t += P2P_THREADS) {
      const int f = t / ny, j = t - f * ny;
      Lc.f[f][(long)ghostL * ny + j] = p2p_load(src + t);
    }
  }
  if (X.sides & 2) {
    const real* src = X.my_recv + ((long)pp * 2 + 1) * X.cap;
    for (int t = threadIdx.x; t < cnt; t += P2P_THREADS) {
      const int f = t / ny, j = t - f * ny;
      Lc.f[f][(long)ghostR * ny + j] = p2p_load(src + t);
    }
  }
  if (threadIdx.x == 0) {
    double m = dt_get(sc, dslot);
    for (int q = 0; q < X.nranks; q++)
      if (q != X.rank) m = fmin(m, p2p_load(X.my_dtr + pp * X.nranks + q));
    sc->dt_bits[dslot] = d_to_bits(m);
  }
}

// Multi-workgroup mailbox exchange, push half (the mechanism step and every
// other p2p exchange with p2p_fuse): each thread loads one boundary value of
// the fields in Lc (column first + o / last - o) and stores it into the
// neighbour's mailbox; the last workgroup publishes and, fold, folds the
// peers' dt into dslot (fx_tail); hf2d_p2p_unpack follows.
// publish = 0: the pushes only (drained); a later hf2d_p2p_finish publishes
// the step -- the mechanism step pushes its edge tiles' halo before its
// interior tiles run.
// One value per thread (135 workgroups on the scramjet's 8-rank strip) pushed
// the 43-field mechanism halo in 7.0 us against 15.4 us with 16 values per
// thread on 9 workgroups (profiles/rejected_variants.md).
__global__ __launch_bounds__(BLOCK) void hf2d_p2p_push(ColList Lc, int first, int last, int ny, int cnt, FusedX X,
                                                      DevScalars* sc, int dslot, int fold, int publish) {
  const unsigned long long seq_prev = *X.seq;
  const int pn = (int)((seq_prev + 1) & 1);
  const long t = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (t < 2L * cnt) {
    const int side = t < cnt ? 0 : 1;
    const int tt = (int)(t - (long)side * cnt), f = tt / ny, j = tt - f * ny;
    real v;
    if ((X.sides & (1 << side)) && !(X.skip & 8))
      v = Lc.f[f][(long)(side == 0 ? first + Lc.o[f] : last - Lc.o[f]) * ny + j];
    // the left neighbour receives "from right", the right one "from left"
    if ((X.sides & (1 << side)) && !(X.skip & 2))
      p2p_store((side == 0 ? X.peer_recv_l + ((long)pn * 2 + 1) * X.cap : X.peer_recv_r + ((long)pn * 2) * X.cap) + tt,
                v);
  }
  vm_drain();
  if (!publish) return;
  __syncthreads();
  if (threadIdx.x < WAVE && !(X.skip & 1)) fx_tail(X, sc, dslot, seq_prev, fold != 0);
}

// One workgroup: publish the step whose halo an earlier hf2d_p2p_push
// (publish = 0) stored, wait for the peers' publication, fold their dt.
__global__ void hf2d_p2p_finish(FusedX X, DevScalars* sc, int dslot) {
  fx_tail(X, sc, dslot, *X.seq, true);   // (one wavefront)
}

// Ghost columns of the HALO_LNS group from the mailbox of the step the fused
// tail just completed (it waited for every peer's flag): entry f of side s
// goes to ghost column ghostL - o[f] / ghostR + o[f] (grid-stride, one value
// per thread).
__global__ __launch_bounds__(BLOCK) void hf2d_p2p_unpack(ColList Lc, int ghostL, int ghostR, int ny, int cnt,
                                                        FusedX X) {
  const int par = (int)(*X.seq & 1);
  for (long t = (long)blockIdx.x * BLOCK + threadIdx.x; t < 2L * cnt; t += (long)gridDim.x * BLOCK) {
    const int side = t < cnt ? 0 : 1;
    if (!(X.sides & (1 << side))) continue;
    const int tt = (int)(t - (long)side * cnt), f = tt / ny, j = tt - f * ny;
    const real v = p2p_load(X.my_recv + ((long)par * 2 + side) * X.cap + tt);
    Lc.f[f][(long)(side == 0 ? ghostL - Lc.o[f] : ghostR + Lc.o[f]) * ny + j] = v;
  }
}
}  // namespace hf2d
