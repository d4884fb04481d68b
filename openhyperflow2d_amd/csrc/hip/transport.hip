// Halo and dt transports of the strip ranks: RCCL, the in-process group and
// the xGMI mailboxes (halo_kernels.hpp), with the host communicators, the halo
// field lists and the overlap of the edge-first steps.

#include "device_impl.hpp"
#include "halo_kernels.hpp"

namespace hf2d {

struct LocalHostComm : Comm {
  std::shared_ptr<LocalGroup> g;
  int r;
  LocalHostComm(std::shared_ptr<LocalGroup> g_, int r_) : g(std::move(g_)), r(r_) {}
  std::vector<std::string> allgather_bytes(const std::string& mine) override {
    g->blobs[r] = mine;
    g->barrier();
    std::vector<std::string> all(g->blobs.begin(), g->blobs.end());
    g->barrier();
    return all;
  }
  int rank() const override { return r; }
  int size() const override { return g->n; }
  real allreduce_min(real v) override { return g->reduce(r, v, 0); }
  real allreduce_sum(real v) override { return g->reduce(r, v, 1); }
  int allreduce_max_int(int v) override { return (int)g->reduce(r, (double)v, 2); }
  void allreduce_residual(ResidualPack& p) override {
    g->packs[r] = p;
    g->barrier();
    ResidualPack a = g->packs[0];
    for (int q = 1; q < g->n; q++) residual_merge_lex(a, g->packs[q]);
    g->barrier();
    p = a;
  }
};

std::shared_ptr<LocalGroup> make_local_group(int n) { return std::make_shared<LocalGroup>(n); }

// RCCL element type of `real` (the halo buffers); the dt words are double /
// 64-bit patterns in both builds and keep ncclDouble / ncclUint64
constexpr ncclDataType_t NCCL_REAL = sizeof(real) == 4 ? ncclFloat : ncclDouble;
static_assert(sizeof(real) == (NCCL_REAL == ncclFloat ? sizeof(float) : sizeof(double)),
              "NCCL_REAL must have the size of real: the halo counts are in elements of real");

// Host-side reductions of the driver over RCCL (output steps only).
struct RcclHostComm : Comm {
  ncclComm_t c;
  hipStream_t st;
  int r, n;
  double* buf = nullptr;
  RcclHostComm(ncclComm_t c_, hipStream_t s_, int r_, int n_) : c(c_), st(s_), r(r_), n(n_) {
    HIP_CHECK(hipMalloc((void**)&buf, sizeof(ResidualPack) * (n + 1) + 64));
  }
  ~RcclHostComm() override { (void)hipFree(buf); }
  int rank() const override { return r; }
  int size() const override { return n; }
  double reduce1(double v, ncclRedOp_t op) {
    HIP_CHECK(hipMemcpyAsync(buf, &v, 8, hipMemcpyHostToDevice, st));
    NCCL_CHECK(ncclAllReduce(buf, buf, 1, ncclDouble, op, c, st));
    HIP_CHECK(hipMemcpyAsync(&v, buf, 8, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return v;
  }
  real allreduce_min(real v) override { return reduce1(v, ncclMin); }
  real allreduce_sum(real v) override { return reduce1(v, ncclSum); }
  int allreduce_max_int(int v) override { return (int)reduce1((double)v, ncclMax); }
  // variable-size all-gather through a device staging buffer: the sizes
  // first, then every rank's bytes padded to the largest (outputs only:
  // row lengths, ghost columns and integral terms once per outer cycle)
  std::vector<std::string> allgather_bytes(const std::string& mine) override {
    long long* dsz = (long long*)buf;
    const long long me = (long long)mine.size();
    HIP_CHECK(hipMemcpyAsync(dsz, &me, sizeof me, hipMemcpyHostToDevice, st));
    NCCL_CHECK(ncclAllGather(dsz, dsz + 1, 1, ncclInt64, c, st));
    std::vector<long long> sz(n);
    HIP_CHECK(hipMemcpyAsync(sz.data(), dsz + 1, sizeof(long long) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    size_t maxb = 1;
    for (long long v : sz) maxb = std::max(maxb, (size_t)v);
    char* stage = nullptr;
    HIP_CHECK(hipMalloc((void**)&stage, maxb * (n + 1)));
    if (me) HIP_CHECK(hipMemcpyAsync(stage, mine.data(), (size_t)me, hipMemcpyHostToDevice, st));
    NCCL_CHECK(ncclAllGather(stage, stage + maxb, maxb, ncclChar, c, st));
    std::string flat(maxb * n, '\0');
    HIP_CHECK(hipMemcpyAsync(&flat[0], stage + maxb, maxb * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(stage));
    std::vector<std::string> all(n);
    for (int q = 0; q < n; q++) all[q] = flat.substr((size_t)q * maxb, (size_t)sz[q]);
    return all;
  }
  void allreduce_residual(ResidualPack& p) override {
    std::vector<ResidualPack> all(n);
    char* dbuf = (char*)buf;
    HIP_CHECK(hipMemcpyAsync(dbuf, &p, sizeof(ResidualPack), hipMemcpyHostToDevice, st));
    NCCL_CHECK(ncclAllGather(dbuf, dbuf + sizeof(ResidualPack), sizeof(ResidualPack), ncclChar, c, st));
    HIP_CHECK(hipMemcpyAsync(all.data(), dbuf + sizeof(ResidualPack), sizeof(ResidualPack) * n, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    ResidualPack a = all[0];
    for (int q = 1; q < n; q++) residual_merge_lex(a, all[q]);
    p = a;
  }
};

std::string DeviceSolver::nccl_unique_id() {
  ncclUniqueId id;
  NCCL_CHECK(ncclGetUniqueId(&id));
  return std::string(id.internal, sizeof(id.internal));
}

void DeviceSolver::init_comm(const std::string& uid, int rank, int nranks) {
  HIP_CHECK(hipSetDevice(dev));
  ncclUniqueId id;
  if (uid.size() != sizeof(id.internal)) throw std::runtime_error("bad RCCL unique id size");
  std::memcpy(id.internal, uid.data(), sizeof(id.internal));
  NCCL_CHECK(ncclCommInitRank(&impl->comm, nranks, id, rank));
  impl->rank = rank;
  impl->nranks = nranks;
  impl->dt_recv = impl->mem.alloc<double>(nranks);
  HIP_CHECK(hipDeviceSynchronize());
  host_comm.reset(new RcclHostComm(impl->comm, impl->stream, rank, nranks));
  comm = host_comm.get();
}

void DeviceSolver::init_local(std::shared_ptr<LocalGroup> g, int rank) {
  impl->local = g;
  impl->rank = rank;
  impl->nranks = g->n;
  impl->dt_recv = impl->mem.alloc<double>(g->n);
  HIP_CHECK(hipDeviceSynchronize());
  host_comm.reset(new LocalHostComm(g, rank));
  comm = host_comm.get();
}

namespace {
struct P2PDesc {
  uint32_t magic;
  int32_t pid, device, rank, nranks, pad;
  uint64_t ptr, bytes;
  char handle[HIP_IPC_HANDLE_SIZE];
};
constexpr uint32_t P2P_MAGIC = 0x68663270;   // "hf2p"
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
}  // namespace

std::string DeviceSolver::p2p_export(int rank, int nranks) {
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  if (m.p2p.base) throw std::runtime_error("p2p_export: mailbox already exported");
  if (nranks < 1 || rank < 0 || rank >= nranks) throw std::runtime_error("p2p_export: bad rank/nranks");
  m.rank = rank;
  m.nranks = nranks;
  Impl::P2P& p = m.p2p;
  p.off_dtr = align_up((size_t)nranks * 8, 256);
  p.off_recv = align_up(p.off_dtr + (size_t)2 * nranks * 8, 256);
  p.bytes = p.off_recv + (size_t)4 * m.halo_cap * sizeof(real);
  void* b = nullptr;
  HIP_CHECK(hipExtMallocWithFlags(&b, p.bytes, hipDeviceMallocFinegrained));
  m.mem.ptrs.push_back(b);
  p.base = (char*)b;
  HIP_CHECK(hipMemset(p.base, 0, p.bytes));
  p.seq = m.mem.alloc<unsigned long long>(1);
  p.done = m.mem.alloc<unsigned>(FX_DONE_WORDS);
  HIP_CHECK(hipDeviceSynchronize());
  P2PDesc d{};
  d.magic = P2P_MAGIC;
  d.pid = (int32_t)getpid();
  d.device = dev;
  d.rank = rank;
  d.nranks = nranks;
  d.ptr = (uint64_t)(uintptr_t)p.base;
  d.bytes = p.bytes;
  hipIpcMemHandle_t h;
  HIP_CHECK(hipIpcGetMemHandle(&h, p.base));
  std::memcpy(d.handle, &h, sizeof(h));
  return std::string((const char*)&d, sizeof d);
}

// One-GPU stand-in for the multi-GPU mailbox exchange (timing only,
// tools/exchange_loopback.py): this strip plays rank `rank` of `nranks`,
// every peer has already published its step (flags at the maximum, dt 1.0),
// and the neighbours' mailboxes are this rank's own (Impl::P2P::push_base:
// the left edge push lands in the left-ghost mailbox, zero-gradient ghosts).
// A step then does every store, publication, poll and ghost staging of a
// real exchange, without a second strip on the GPU and without waiting --
// what remains is the exchange's own cost on this device (the xGMI link
// latency is not in it).
void DeviceSolver::p2p_loopback(int rank, int nranks) {
  if (nranks < 2 || rank < 0 || rank >= nranks) throw std::runtime_error("p2p_loopback: bad rank/nranks");
  (void)p2p_export(rank, nranks);
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  Impl::P2P& p = m.p2p;
  p.peer_base.assign(nranks, p.base);
  std::vector<unsigned long long> flags(nranks, ~0ull);
  flags[rank] = 0;
  std::vector<double> dtr(2 * (size_t)nranks, 1.0);
  HIP_CHECK(hipMemcpy(p.base, flags.data(), nranks * sizeof(unsigned long long), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(p.base + p.off_dtr, dtr.data(), dtr.size() * sizeof(double), hipMemcpyHostToDevice));
  std::vector<unsigned long long*> fl(nranks, (unsigned long long*)p.base);
  std::vector<double*> dr(nranks, (double*)(p.base + p.off_dtr));
  p.d_flags = m.mem.alloc<unsigned long long*>(nranks);
  p.d_dtr = m.mem.alloc<double*>(nranks);
  if (!m.lc_dev) m.lc_dev = m.mem.alloc<ColList>(2);
  HIP_CHECK(hipMemcpy(p.d_flags, fl.data(), nranks * sizeof(void*), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(p.d_dtr, dr.data(), nranks * sizeof(void*), hipMemcpyHostToDevice));
  p.loop = true;
  p.on = true;
}

void DeviceSolver::p2p_import(const std::vector<std::string>& descs) {
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  Impl::P2P& p = m.p2p;
  if (!p.base) throw std::runtime_error("p2p_import before p2p_export");
  if ((int)descs.size() != m.nranks) throw std::runtime_error("p2p_import: need one descriptor per rank");
  if (p2p_queue_check) {
    // In-process ranks on one device (virtual ranks: tests, one-GPU boxes).
    // Every rank's exchange kernel ends in a workgroup that spins until all
    // peers have published, so the ranks' kernels must run concurrently.  HIP
    // maps a process's streams onto at most GPU_MAX_HW_QUEUES hardware queues
    // per device (default 4) and past that puts two streams on one queue,
    // whose packets run in order: a spinning kernel then holds back the peer
    // kernel queued behind it until the bounded wait expires ("rank 0 timed
    // out waiting for its peers", the round-5 4-rank probe).  Measured on
    // MI355X (tools/hwq_probe.py, profiles/hwq_probe_r06.md): n ranks in one
    // process co-schedule iff GPU_MAX_HW_QUEUES >= n + 1 (3 and 4 queues,
    // 4 and 8, 8 and 16 pass; 4 and 4, 8 and 8 time out).  Separate
    // processes (the multi-GPU layout) have queues of their own.
    int local = 0;
    for (const std::string& s : descs) {
      P2PDesc d;
      if (s.size() != sizeof d) continue;
      std::memcpy(&d, s.data(), sizeof d);
      local += (d.pid == (int32_t)getpid() && d.device == dev) ? 1 : 0;
    }
    const char* q = std::getenv("GPU_MAX_HW_QUEUES");
    const int hwq = (q && std::atoi(q) > 0) ? std::atoi(q) : 4;
    if (local > 1 && local + 1 > hwq)
      throw std::runtime_error("p2p_import: " + std::to_string(local) + " mailbox ranks share device " +
                               std::to_string(dev) + " in one process, which has " + std::to_string(hwq) +
                               " HIP hardware queues (GPU_MAX_HW_QUEUES); their exchange kernels wait for each "
                               "other, so each rank needs a queue of its own plus one for the default stream: set "
                               "GPU_MAX_HW_QUEUES >= " + std::to_string(local + 1) +
                               " before the first HIP call, or run the ranks as separate processes");
  }
  p.peer_base.assign(m.nranks, nullptr);
  for (int q = 0; q < m.nranks; q++) {
    P2PDesc d;
    if (descs[q].size() != sizeof d) throw std::runtime_error("p2p_import: bad descriptor size");
    std::memcpy(&d, descs[q].data(), sizeof d);
    if (d.magic != P2P_MAGIC || d.rank != q || d.nranks != m.nranks || d.bytes != p.bytes)
      throw std::runtime_error("p2p_import: descriptor mismatch (rank " + std::to_string(q) + ")");
    if (q == m.rank) {
      p.peer_base[q] = p.base;
    } else if (d.pid == (int32_t)getpid()) {   // in-process virtual rank
      if (d.device != dev) {
        const hipError_t e = hipDeviceEnablePeerAccess(d.device, 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_CHECK(e);
        (void)hipGetLastError();
      }
      p.peer_base[q] = (char*)(uintptr_t)d.ptr;
    } else {
      hipIpcMemHandle_t h;
      std::memcpy(&h, d.handle, sizeof h);
      void* ptr = nullptr;
      HIP_CHECK(hipIpcOpenMemHandle(&ptr, h, hipIpcMemLazyEnablePeerAccess));
      p.opened.push_back(ptr);
      p.peer_base[q] = (char*)ptr;
    }
  }
  std::vector<unsigned long long*> fl(m.nranks);
  std::vector<double*> dr(m.nranks);
  for (int q = 0; q < m.nranks; q++) {
    fl[q] = (unsigned long long*)p.peer_base[q];
    dr[q] = (double*)(p.peer_base[q] + p.off_dtr);
  }
  p.d_flags = m.mem.alloc<unsigned long long*>(m.nranks);
  p.d_dtr = m.mem.alloc<double*>(m.nranks);
  if (!m.lc_dev) m.lc_dev = m.mem.alloc<ColList>(2);   // (fused lean N-S ghost prologue lists)
  HIP_CHECK(hipDeviceSynchronize());
  HIP_CHECK(hipMemcpy(p.d_flags, fl.data(), m.nranks * sizeof(void*), hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(p.d_dtr, dr.data(), m.nranks * sizeof(void*), hipMemcpyHostToDevice));
  p.on = m.nranks > 1;
}

bool DeviceSolver::p2p_active() const { return impl->p2p.on; }

void DeviceSolver::p2p_set(bool on) {
  flush_pending();
  p2p_complete();
  lns_last_valid = false;
  if (on && (impl->p2p.peer_base.empty() || impl->nranks < 2)) throw std::runtime_error("p2p_set: no imported peers");
  impl->p2p.on = on;
  graph.reset();   // captured exchanges belong to the old transport
}

int DeviceSolver::comm_rank() const { return impl->rank; }
int DeviceSolver::comm_size() const { return impl->nranks; }

// Halo exchange of one field group with RCCL send/recv to the strip
// neighbours (rank-1 owns the columns to the left).  dt_slot >= 0: the
// same RCCL group also sends this rank's dt of that slot to every other rank
// and unpack folds the MIN in -- one grouped p2p launch per step instead of a
// send/recv group plus an all-reduce.
// device columns of the fields a halo group carries (pack order)
int DeviceSolver::split_mode() const {
  return impl->mech ? SK_MECH : (cs.cfg.ProblemType == SM_NS && sgl) ? sk_mode : SK_GENERIC;
}

void DeviceSolver::halo_fields(int group, std::vector<real*>& f, bool full) const {
  std::vector<unsigned char> o;
  halo_fields(group, f, o, full);
}

// HALO_LNS: lean N-S / mechanism strips (two ghost columns): what the next
// lean step reads of them -- the inner ghost column is a ring cell (its fill
// reads its predicted state, lagged primitives, transport and thermodynamic
// state), the outer one only the neighbour values of that fill (state,
// species, lagged U, V, T).  For the buffer parities sb / pb / cb / ds (a
// fused step lists its post-step buffers before it flips the members).
void DeviceSolver::halo_fields_lns(std::vector<real*>& f, std::vector<unsigned char>& o, int sb, int pb, int cb,
                                   int ds) const {
  const Impl& m = *impl;
  const long N = h.N;
  f.clear();
  o.clear();
  auto two = [&](real* p) {
    f.push_back(p);
    o.push_back(0);
    f.push_back(p);
    o.push_back(1);
  };
  auto one = [&](real* p) {
    f.push_back(p);
    o.push_back(0);
  };
  for (int k = 0; k < NEQ; k++)
    if (sk_live(m.mech ? SK_MECH : sk_mode, k)) two(m.S[1 - sb] + (long)k * N);
  two(m.U[1 - pb]);
  two(m.V[1 - pb]);
  two(m.Tg[1 - pb]);
  const Impl::Levels x = m.levels();
  one(x.mu[1 - cb]);
  one(x.lam[1 - cb]);
  one(x.mu_t[1 - cb]);
  one(x.CP[1 - cb]);
  one(x.kk[1 - cb]);
  if (m.mech) {
    one(x.p[1 - cb]);
    one(m.Tst[1 - cb]);
    for (int q = 0; q < m.nsp; q++) two(m.Ys[sb] + (long)q * N);
  }
  if (any_cauchy_x) {   // dS/dx of the ghost column (Cauchy neighbours of the edge cells)
    for (int k = 0; k < NEQ; k++)
      if (sk_live(m.mech ? SK_MECH : sk_mode, k)) one(m.dSdx[ds] + (long)k * N);
    if (m.dSdxs[0])
      for (int q = 0; q < m.nsp; q++) one(m.dSdxs[ds] + (long)q * N);
  }
}

void DeviceSolver::halo_fields(int group, std::vector<real*>& f, std::vector<unsigned char>& o, bool full) const {
  if (group == CpuSolver::HALO_LNS) return halo_fields_lns(f, o, sbuf, pbuf, cbuf, dsbuf);
  const Impl& m = *impl;
  const long N = h.N;
  f.clear();
  o.clear();
  full = full || !halo_compact;
  const int mode = split_mode();
  auto add_eq = [&](real* base) {
    for (int k = 0; k < NEQ; k++) f.push_back(base + (long)k * N);
  };
  if (group == CpuSolver::HALO_LEAN) {
    // single gas: the species (and their pre-chemistry copies) are +0 on
    // every rank; dS/dx only travels if some node applies d2/dx2 = 0
    const bool sg = lean_sg && lean_sg_ok;
    for (int k = 0; k < (sg ? 4 : 4 + NCOMP); k++) f.push_back(m.S[sbuf] + (long)k * N);
    if (!sg)
      for (int k = 0; k < NCOMP; k++) f.push_back(m.Spre[pbuf] + (long)k * N);
    f.push_back(m.U[pbuf]);
    f.push_back(m.V[pbuf]);
    f.push_back(m.P2[pbuf]);
    if (lean_has_cauchy_x) add_eq(m.dSdx[dsbuf]);
  } else if (group == CpuSolver::HALO_MID) {
    // the predicted state as the N-S fill reads it of an x neighbour
    // (stepkern.hpp fill_compute: Sn of rho, the species slots, k and eps);
    // mechanism strips also react their ghost columns, which reads rho, rhoU,
    // rhoV and rhoE (chem_fast_dev.hpp chem_cell)
    for (int k = 0; k < NEQ; k++)
      if (full || k == 0 || (mode == SK_MECH && k < 4) || (k >= 4 && sk_live(mode, k)))
        f.push_back(m.S[1 - sbuf] + (long)k * N);
    for (int q = 0; q < m.nsp; q++) f.push_back(m.Ys[1 - sbuf] + (long)q * N);
  } else if (group == CpuSolver::HALO_QDIR) {
    for (int d = 0; d < 4; d++) f.push_back(m.qdir + (long)d * N);
  } else {
    // what the next split step reads of a ghost column: the predictor's S
    // and x flux A of the live equations (stepkern.hpp predict_core: SL/SR,
    // AL/AR; the y flux B only along the own column), dS/dx only where a node
    // applies d2/dx2 = 0, the fill's previous U/V/T and the wall heat flux's
    // conductivities; the mechanism species block likewise
    for (int k = 0; k < NEQ; k++)
      if (full || sk_live(mode, k)) f.push_back(m.S[sbuf] + (long)k * N);
    for (int k = 0; k < NEQ; k++)
      if (full || sk_live(mode, k)) f.push_back(m.A[abuf] + (long)k * N);
    if (full) add_eq(m.B[abuf]);
    if (full || any_cauchy_x)
      for (int k = 0; k < NEQ; k++)
        if (full || sk_live(mode, k)) f.push_back(m.dSdx[dsbuf] + (long)k * N);
    f.push_back(m.U[pbuf]);
    f.push_back(m.V[pbuf]);
    f.push_back(m.Tg[pbuf]);
    f.push_back(m.lam);
    f.push_back(m.lam_t);
    for (int q = 0; q < m.nsp; q++) {
      f.push_back(m.Ys[sbuf] + (long)q * N);
      f.push_back(m.As + (long)q * N);
      if (full) f.push_back(m.Bs + (long)q * N);
      if (m.dSdxs[0] && (full || any_cauchy_x)) f.push_back(m.dSdxs[dsbuf] + (long)q * N);
    }
  }
}

void DeviceSolver::exchange(int group, int dt_slot, void* on_stream, bool full) {
  Impl& m = *impl;
  p2p_complete();
  lns_last_valid = false;
  if ((!m.comm && !m.local && !m.p2p.on) || m.nranks == 1) return;
  const int ny = h.ny;
  std::vector<real*> fl;
  std::vector<unsigned char> fo;
  halo_fields(group, fl, fo, full);
  if (group == CpuSolver::HALO_STATE) ghost_mode = (full || !halo_compact) ? -1 : split_mode();
  if (group == CpuSolver::HALO_LNS) ghost_stale = true;   // lean representation in the ghosts
  else if (group == CpuSolver::HALO_STATE) ghost_stale = false;
  if (fl.size() > (size_t)MAX_HALO_FIELDS) throw std::runtime_error("halo: too many exchanged fields");
  ColList L;
  L.nf = (int)fl.size();
  for (int k = 0; k < L.nf; k++) {
    L.f[k] = fl[k];
    L.o[k] = k < (int)fo.size() ? fo[k] : 0;
  }
  const int cnt = L.nf * ny;
  const unsigned nb2 = (unsigned)((2 * cnt + BLOCK - 1) / BLOCK);
  const int first = l_off, last = l_off + (gi1 - gi0) - 1;
  const bool has_left = gi0 > 0, has_right = gi1 < cs.J.nx;
  const int sides = (has_left ? 1 : 0) | (has_right ? 2 : 0);
  hipStream_t st = on_stream ? (hipStream_t)on_stream : m.stream;
  if (m.p2p.on && p2p_fuse) {
    // multi-workgroup push (the last workgroup publishes, waits and folds the
    // dt), then the multi-workgroup unpack: no single-workgroup copy of the
    // 23-43-field N-S / mechanism halos on the step's critical path
    if (L.nf * ny > m.halo_cap) throw std::runtime_error("p2p halo exceeds mailbox capacity");
    p2p_push(L, st, dt_slot >= 0 ? dt_slot : 0, dt_slot >= 0 ? 1 : 0, 1);
    p2p_mwg_exchanges++;
    if (group == CpuSolver::HALO_LNS && dt_slot >= 0 && lns_ghost_prologue && !on_stream) {
      // the mechanism step's halo: the next mechanism step's edge tiles
      // unpack it (fx_ghost_prologue), any other consumer p2p_complete
      m.lns_pend = L;
      lns_ghost_pending = lns_last_valid = true;
      return;
    }
    p2p_unpack(L, st);
    return;
  }
  if (m.p2p.on) {
    if (L.nf * ny > m.halo_cap) throw std::runtime_error("p2p halo exceeds mailbox capacity");
    Impl::P2P& p = m.p2p;
    P2PArgs a;
    a.L = L;
    a.first = first;
    a.last = last;
    a.ghostL = l_off - 1;
    a.ghostR = l_off + (gi1 - gi0);
    a.ny = ny;
    a.cnt = cnt;
    a.sides = sides;
    a.cap = m.halo_cap;
    a.peer_recv_l = has_left ? p.push_base(0, m.rank, m.halo_cap) : nullptr;
    a.peer_recv_r = has_right ? p.push_base(1, m.rank, m.halo_cap) : nullptr;
    a.my_recv = (real*)(p.base + p.off_recv);
    a.peer_flags = p.d_flags;
    a.peer_dtr = p.d_dtr;
    a.my_flags = (unsigned long long*)p.base;
    a.my_dtr = (double*)(p.base + p.off_dtr);
    a.seq = p.seq;
    a.sc = m.sc;
    a.dslot = dt_slot >= 0 ? dt_slot : 0;
    a.fold_dt = dt_slot >= 0 ? 1 : 0;
    a.rank = m.rank;
    a.nranks = m.nranks;
    hipLaunchKernelGGL(hf2d_p2p_xchg, dim3(1), dim3(P2P_THREADS), 0, m.stream, a);
    HIP_CHECK(hipGetLastError());
    return;
  }
  const bool gather_dt = dt_slot >= 0;
  hipLaunchKernelGGL(hf2d_pack2, dim3(std::max(nb2, 1u)), dim3(BLOCK), 0, st, L, first, last, ny, m.halo_send[0],
                     m.halo_send[1], sides, m.sc, gather_dt ? dt_slot : -1);
  unsigned long long* my_dt = gather_dt ? &m.sc->dt_bits[dt_slot] : nullptr;
  if (m.local) {
    LocalGroup& g = *m.local;
    HIP_CHECK(hipStreamSynchronize(st));
    g.send_l[m.rank] = m.halo_send[0];
    g.send_r[m.rank] = m.halo_send[1];
    g.dt_src[m.rank] = my_dt;
    g.barrier();
    if (gather_dt)
      for (int q = 0; q < m.nranks; q++)
        if (q != m.rank)
          HIP_CHECK(hipMemcpyAsync(m.dt_recv + q, g.dt_src[q], sizeof(double), hipMemcpyDeviceToDevice, st));
    if (has_left)
      HIP_CHECK(hipMemcpyAsync(m.halo_recv[0], g.send_r[m.rank - 1], (size_t)cnt * sizeof(real),
                               hipMemcpyDeviceToDevice, st));
    if (has_right)
      HIP_CHECK(hipMemcpyAsync(m.halo_recv[1], g.send_l[m.rank + 1], (size_t)cnt * sizeof(real),
                               hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));
    g.barrier();
  } else {
  NCCL_CHECK(ncclGroupStart());
  if (has_left) {
    NCCL_CHECK(ncclSend(m.halo_send[0], cnt, NCCL_REAL, m.rank - 1, m.comm, st));
    NCCL_CHECK(ncclRecv(m.halo_recv[0], cnt, NCCL_REAL, m.rank - 1, m.comm, st));
  }
  if (has_right) {
    NCCL_CHECK(ncclSend(m.halo_send[1], cnt, NCCL_REAL, m.rank + 1, m.comm, st));
    NCCL_CHECK(ncclRecv(m.halo_recv[1], cnt, NCCL_REAL, m.rank + 1, m.comm, st));
  }
  if (gather_dt)
    for (int q = 0; q < m.nranks; q++)
      if (q != m.rank) {
        NCCL_CHECK(ncclSend(my_dt, 1, ncclDouble, q, m.comm, st));
        NCCL_CHECK(ncclRecv(m.dt_recv + q, 1, ncclDouble, q, m.comm, st));
      }
  NCCL_CHECK(ncclGroupEnd());
  }
  hipLaunchKernelGGL(hf2d_unpack2, dim3(std::max(nb2, 1u)), dim3(BLOCK), 0, st, L, l_off - 1, l_off + (gi1 - gi0), ny,
                     m.halo_recv[0], m.halo_recv[1], sides, m.sc, gather_dt ? dt_slot : 0, m.dt_recv,
                     gather_dt ? m.nranks : 0, m.rank);
  HIP_CHECK(hipGetLastError());
}

namespace {
struct P2PProbe {
  int32_t rank, sides, err, pad;
  uint64_t sent_l, sent_r, recv_l, recv_r;
  double dt;
};
uint64_t fnv1a(const std::vector<real>& v) {
  uint64_t h = 1469598103934665603ULL;
  const unsigned char* p = (const unsigned char*)v.data();
  for (size_t k = 0; k < v.size() * sizeof(real); k++) h = (h ^ p[k]) * 1099511628211ULL;
  return h;
}
constexpr double PROBE_DT0 = 1.0, PROBE_DT_STEP = 0.25;   // rank r offers 1 + r/4: the MIN is 1
}  // namespace

std::string DeviceSolver::p2p_probe() {
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  if (!m.p2p.on) throw std::runtime_error("p2p_probe: p2p transport not active");
  hipStream_t st = m.stream;
  const int ny = h.ny;
  const int first = l_off, last = l_off + (gi1 - gi0) - 1, gl = l_off - 1, gr = l_off + (gi1 - gi0);
  const bool has_left = gi0 > 0, has_right = gi1 < cs.J.nx;
  std::vector<real*> fl;
  halo_fields(CpuSolver::HALO_STATE, fl);
  DevScalars saved;
  HIP_CHECK(hipMemcpyAsync(&saved, m.sc, sizeof saved, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  // poison the ghost columns (all-ones bytes: NaN) so a lost delivery shows
  for (real* f : fl) {
    if (has_left) HIP_CHECK(hipMemsetAsync(f + (long)gl * ny, 0xFF, ny * sizeof(real), st));
    if (has_right) HIP_CHECK(hipMemsetAsync(f + (long)gr * ny, 0xFF, ny * sizeof(real), st));
  }
  const unsigned long long tag = [&] {
    const double d = PROBE_DT0 + PROBE_DT_STEP * m.rank;
    unsigned long long b;
    std::memcpy(&b, &d, sizeof b);
    return b;
  }();
  DevScalars tagged = saved;
  dt_set_host(tagged, 0, tag);
  HIP_CHECK(hipMemcpyAsync(m.sc, &tagged, sizeof tagged, hipMemcpyHostToDevice, st));
  HIP_CHECK(hipStreamSynchronize(st));
  exchange(CpuSolver::HALO_STATE, 0);
  auto column = [&](int col) {
    std::vector<real> v(fl.size() * (size_t)ny);
    for (size_t k = 0; k < fl.size(); k++)
      HIP_CHECK(hipMemcpyAsync(v.data() + k * ny, fl[k] + (long)col * ny, ny * sizeof(real), hipMemcpyDeviceToHost, st));
    return v;
  };
  std::vector<real> sl, sr, rl, rr;
  if (has_left) {
    sl = column(first);
    rl = column(gl);
  }
  if (has_right) {
    sr = column(last);
    rr = column(gr);
  }
  DevScalars after;
  HIP_CHECK(hipMemcpyAsync(&after, m.sc, sizeof after, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipStreamSynchronize(st));
  HIP_CHECK(hipMemcpyAsync(m.sc, &saved, sizeof saved, hipMemcpyHostToDevice, st));   // dt slots, error flag
  HIP_CHECK(hipStreamSynchronize(st));
  P2PProbe b{};
  b.rank = m.rank;
  b.sides = (has_left ? 1 : 0) | (has_right ? 2 : 0);
  b.err = after.neg_T & 2;
  b.sent_l = has_left ? fnv1a(sl) : 0;
  b.sent_r = has_right ? fnv1a(sr) : 0;
  b.recv_l = has_left ? fnv1a(rl) : 0;
  b.recv_r = has_right ? fnv1a(rr) : 0;
  const unsigned long long adt = dt_get_host(after, 0);
  std::memcpy(&b.dt, &adt, sizeof b.dt);
  return std::string((const char*)&b, sizeof b);
}

bool DeviceSolver::p2p_probe_ok(const std::vector<std::string>& blobs, int rank, std::string* why) {
  auto bad = [&](const std::string& w) {
    if (why) *why = w;
    return false;
  };
  std::vector<P2PProbe> p(blobs.size());
  for (size_t q = 0; q < blobs.size(); q++) {
    if (blobs[q].size() != sizeof(P2PProbe)) return bad("probe blob of rank " + std::to_string(q) + " missing");
    std::memcpy(&p[q], blobs[q].data(), sizeof(P2PProbe));
  }
  const int n = (int)p.size();
  (void)rank;
  for (int q = 0; q < n; q++) {   // every rank judges all ranks: the verdict is identical everywhere
    if (p[q].rank != q) return bad("probe rank mismatch");
    if (p[q].err) return bad("rank " + std::to_string(q) + " timed out waiting for its peers");
    if (p[q].dt != PROBE_DT0) return bad("rank " + std::to_string(q) + " folded dt " + std::to_string(p[q].dt));
    if ((p[q].sides & 1) && (q == 0 || p[q].recv_l != p[q - 1].sent_r))
      return bad("left halo of rank " + std::to_string(q) + " differs from what rank " + std::to_string(q - 1) + " sent");
    if ((p[q].sides & 2) && (q == n - 1 || p[q].recv_r != p[q + 1].sent_l))
      return bad("right halo of rank " + std::to_string(q) + " differs from what rank " + std::to_string(q + 1) + " sent");
  }
  return true;
}

// p2p failed validation: RCCL (or the in-process group) carries the halos
// from now on; refill the ghost columns the probe poisoned
void DeviceSolver::p2p_fallback() {
  p2p_set(false);
  exchange(CpuSolver::HALO_STATE, -1);
  HIP_CHECK(hipStreamSynchronize(impl->stream));
}

// The global dt MIN alone (comm-overlap steps exchange the halo before the
// interior tiles have produced their dt): RCCL all-reduce (MIN) on the IEEE
// bits of the positive doubles, or the in-process group's device copies.
void DeviceSolver::exchange_dt(int dt_slot) {
  Impl& m = *impl;
  if (m.nranks <= 1) return;
  unsigned long long* my_dt = &m.sc->dt_bits[dt_slot];
  hipLaunchKernelGGL(hf2d_dt_commit, dim3(1), dim3(64), 0, m.stream, m.sc, dt_slot);
  HIP_CHECK(hipGetLastError());
  if (m.comm) {
    NCCL_CHECK(ncclAllReduce(my_dt, my_dt, 1, ncclUint64, ncclMin, m.comm, m.stream));
    return;
  }
  if (!m.local) throw std::runtime_error("exchange_dt: no transport");
  LocalGroup& g = *m.local;
  HIP_CHECK(hipStreamSynchronize(m.stream));
  g.dt_src[m.rank] = my_dt;
  g.barrier();
  for (int q = 0; q < m.nranks; q++)
    if (q != m.rank)
      HIP_CHECK(hipMemcpyAsync(m.dt_recv + q, g.dt_src[q], sizeof(double), hipMemcpyDeviceToDevice, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  g.barrier();
  hipLaunchKernelGGL(hf2d_fold_dt, dim3(1), dim3(64), 0, m.stream, m.sc, dt_slot, m.dt_recv, m.nranks, m.rank);
  HIP_CHECK(hipGetLastError());
}

// Device copy of the fused-exchange arguments for the tile kernels (uploaded
// when they change: at the first fused step, which is never inside a graph
// capture -- the lean entry step runs eagerly)
const FusedX* DeviceSolver::fx_device(const FusedX& X) {
  Impl& m = *impl;
  if (!m.fx_dev) m.fx_dev = m.mem.alloc<FusedX>(1);
  if (!m.fx_dev_valid || std::memcmp(&m.fx_dev_host, &X, sizeof X) != 0) {
    hipStreamCaptureStatus cs_ = hipStreamCaptureStatusNone;
    HIP_CHECK(hipStreamIsCapturing(m.stream, &cs_));
    if (cs_ != hipStreamCaptureStatusNone) throw std::runtime_error("fused exchange arguments changed inside a graph capture");
    HIP_CHECK(hipStreamSynchronize(m.stream));
    HIP_CHECK(hipMemcpy(m.fx_dev, &X, sizeof X, hipMemcpyHostToDevice));
    m.fx_dev_host = X;
    m.fx_dev_valid = true;
  }
  return m.fx_dev;
}

// Device copy of a HALO_LNS list for a fused step's ghost prologue (the two
// buffer parities' lists are uploaded once, outside graph captures; nullptr
// when a new list shows up inside a capture: that step unpacks separately)
namespace {
bool same_list(const ColList& a, const ColList& b) {   // (the entries only: padding bytes are unspecified)
  if (a.nf != b.nf) return false;
  for (int k = 0; k < a.nf; k++)
    if (a.f[k] != b.f[k] || a.o[k] != b.o[k]) return false;
  return true;
}
}  // namespace

const ColList* DeviceSolver::lc_device(const ColList& L) {
  Impl& m = *impl;
  if (!m.lc_dev) return nullptr;   // (allocated by p2p_import)
  for (int k = 0; k < 2; k++)
    if (m.lc_valid[k] && same_list(m.lc_host[k], L)) return m.lc_dev + k;
  // a slot is written once (a captured window may reference it); the two
  // buffer parities' lists fill both, anything else unpacks separately
  if (m.lc_next >= 2) return nullptr;
  hipStreamCaptureStatus cs_ = hipStreamCaptureStatusNone;
  HIP_CHECK(hipStreamIsCapturing(m.stream, &cs_));
  if (cs_ != hipStreamCaptureStatusNone) return nullptr;
  const int k = m.lc_next++;
  m.lc_host[k] = L;
  // stream-ordered from the persistent host copy: no host wait in the step
  HIP_CHECK(hipMemcpyAsync(m.lc_dev + k, &m.lc_host[k], sizeof L, hipMemcpyHostToDevice, m.stream));
  m.lc_valid[k] = true;
  return m.lc_dev + k;
}

// Tail phase clocks of the last FX_TRACE_N fused exchanges (HF2D_FX_SKIP bit
// 4 on a loopback run): FX_TRACE_W words per step, zero where none ran.
std::vector<unsigned long long> DeviceSolver::fx_trace() {
  flush_pending();
  Impl& m = *impl;
  std::vector<unsigned long long> v((size_t)FX_TRACE_N * FX_TRACE_W, 0ull);
  if (!m.p2p.done) return v;
  HIP_CHECK(hipStreamSynchronize(m.stream));
  HIP_CHECK(hipMemcpy(v.data(), m.p2p.done + (DT_SHARDS + 1) * FX_DONE_STRIDE, v.size() * sizeof(unsigned long long),
                      hipMemcpyDeviceToHost));
  return v;
}

FusedX DeviceSolver::fused_args() const {
  const Impl& m = *impl;
  const Impl::P2P& p = m.p2p;
  const bool has_left = gi0 > 0, has_right = gi1 < cs.J.nx;
  FusedX X{};
  X.peer_recv_l = has_left ? p.push_base(0, m.rank, m.halo_cap) : nullptr;
  X.peer_recv_r = has_right ? p.push_base(1, m.rank, m.halo_cap) : nullptr;
  X.my_recv = (const real*)(p.base + p.off_recv);
  X.peer_flags = p.d_flags;
  X.peer_dtr = p.d_dtr;
  X.my_flags = (const unsigned long long*)p.base;
  X.my_dtr = (const double*)(p.base + p.off_dtr);
  X.seq = p.seq;
  X.done = p.done;
  X.cap = m.halo_cap;
  X.rank = m.rank;
  X.nranks = m.nranks;
  X.sides = (has_left ? 1 : 0) | (has_right ? 2 : 0);
  X.on = 1;
  X.skip = m.p2p.loop ? fx_skip : 0;   // (loopback timing runs only)
  X.edge_first = fx_edge_first;
  X.count1 = fx_count1;
  return X;
}

// The multi-workgroup mailbox exchange in its three launches (halo_kernels.hpp),
// for the list L of this strip's columns: the edge columns into the
// neighbours' mailboxes (finish: the last workgroup also publishes, waits and,
// with fold_dt, folds the peers' dt into dt_slot); that tail alone, after
// kernels of the caller's that follow a push without it; mailbox -> ghost columns.
void DeviceSolver::p2p_push(const ColList& L, void* on_stream, int dt_slot, int fold_dt, int finish) {
  Impl& m = *impl;
  const int cnt = L.nf * h.ny;
  hipLaunchKernelGGL(hf2d_p2p_push, dim3((unsigned)std::max(1, (2 * cnt + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0,
                     (hipStream_t)on_stream, L, l_off, l_off + (gi1 - gi0) - 1, h.ny, cnt, fused_args(), m.sc, dt_slot,
                     fold_dt, finish);
  HIP_CHECK(hipGetLastError());
}

void DeviceSolver::p2p_finish(int dt_slot) {
  Impl& m = *impl;
  hipLaunchKernelGGL(hf2d_p2p_finish, dim3(1), dim3(WAVE), 0, m.stream, fused_args(), m.sc, dt_slot);
  HIP_CHECK(hipGetLastError());
}

void DeviceSolver::p2p_unpack(const ColList& L, void* on_stream) {
  const int cnt = L.nf * h.ny;
  hipLaunchKernelGGL(hf2d_p2p_unpack, dim3((unsigned)std::max(1, std::min((2 * cnt + BLOCK - 1) / BLOCK, 1024))),
                     dim3(BLOCK), 0, (hipStream_t)on_stream, L, l_off - 1, l_off + (gi1 - gi0), h.ny, cnt,
                     fused_args());
  HIP_CHECK(hipGetLastError());
}

// After fused-exchange steps the newest ghost columns and the peers' dt live
// only in the mailbox: materialise them before any other consumer.
void DeviceSolver::p2p_complete(bool keep_lns) {
  Impl& m = *impl;
  if (lns_ghost_pending && !keep_lns) {
    // the last fused lean N-S / mechanism step's halo: mailbox -> ghost columns
    lns_ghost_pending = false;
    p2p_unpack(m.lns_pend, m.stream);
  }
  if (!fx_pending) return;
  fx_pending = false;
  const long N = h.N;
  ColList L;
  L.nf = 0;
  const bool sg = lean_sg && lean_sg_ok;
  for (int k = 0; k < (sg ? 4 : 4 + NCOMP); k++) L.f[L.nf++] = m.S[sbuf] + (long)k * N;
  if (!sg)
    for (int k = 0; k < NCOMP; k++) L.f[L.nf++] = m.Spre[pbuf] + (long)k * N;
  L.f[L.nf++] = m.U[pbuf];
  L.f[L.nf++] = m.V[pbuf];
  L.f[L.nf++] = m.P2[pbuf];
  hipLaunchKernelGGL(hf2d_p2p_complete, dim3(1), dim3(P2P_THREADS), 0, m.stream, L, l_off - 1, l_off + (gi1 - gi0), h.ny,
                     L.nf * h.ny,
                     fused_args(), m.sc, (int)(nstep % 3));
  HIP_CHECK(hipGetLastError());
}

// Edge-first steps of the RCCL / in-process transports: the comm stream and
// the two events that order it against the step's stream.
void DeviceSolver::overlap_streams() {
  Impl& m = *impl;
  if (m.comm_stream) return;
  HIP_CHECK(hipStreamCreateWithFlags(&m.comm_stream, hipStreamNonBlocking));
  HIP_CHECK(hipEventCreateWithFlags(&m.ev_edge, hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&m.ev_halo, hipEventDisableTiming));
}

// The new state's halo of an edge-first step on the comm stream, after the
// edge part (ev_edge, recorded on the step's stream) and while the interior
// part runs, then the dt MIN over the ranks into slot_next.
void DeviceSolver::overlap_exchange(int group, int slot_next) {
  Impl& m = *impl;
  if (m.local) {
    // in-process group: the host orders the two streams (waits on it).
    // Device-side cross-stream waits would put barrier packets in hardware
    // queues that several virtual ranks' streams share, and a wait cycle
    // across those queues can deadlock.
    HIP_CHECK(hipEventSynchronize(m.ev_edge));
    exchange(group, -1, (void*)m.comm_stream);
    HIP_CHECK(hipStreamSynchronize(m.comm_stream));
  } else {
    HIP_CHECK(hipStreamWaitEvent(m.comm_stream, m.ev_edge, 0));
    exchange(group, -1, (void*)m.comm_stream);
    HIP_CHECK(hipEventRecord(m.ev_halo, m.comm_stream));
    HIP_CHECK(hipStreamWaitEvent(m.stream, m.ev_halo, 0));
  }
  exchange_dt(slot_next);
  overlap_steps++;
}

// The HALO_LNS pointers of the post-step buffers (a fused step pushes the
// state it is about to write).
ColList DeviceSolver::lns_post_list(const char* what) const {
  std::vector<real*> fl;
  std::vector<unsigned char> fo;
  halo_fields_lns(fl, fo, 1 - sbuf, 1 - pbuf, 1 - cbuf, 1 - dsbuf);
  if (fl.size() > (size_t)MAX_HALO_FIELDS || (long)fl.size() * h.ny > impl->halo_cap)
    throw std::runtime_error(std::string(what) + " halo exceeds the mailbox capacity");
  ColList Lc{};
  Lc.nf = (int)fl.size();
  for (int k = 0; k < Lc.nf; k++) {
    Lc.f[k] = fl[k];
    Lc.o[k] = fo[k];
  }
  return Lc;
}

// The previous fused step's halo is still in the mailbox: this step's edge
// tiles copy it into the ghost columns they read (fx_ghost_prologue) instead
// of a separate unpack launch.  Valid whenever the mailbox's last
// publication was a fused lean N-S / mechanism step: its parity stays
// untouched until this step publishes, so the copy is exact even if
// p2p_complete already unpacked it.  nullptr (a list new inside a capture,
// or no such publication): the separate unpack of p2p_complete.
const ColList* DeviceSolver::claim_ghost_prologue() {
  if (!lns_prev_valid || !lns_ghost_prologue) return nullptr;
  const ColList* Lg = lc_device(impl->lns_pend);
  if (Lg) {
    lns_ghost_pending = false;
    lns_pro_uses++;
    lns_prologue_steps++;
  }
  return Lg;
}

}  // namespace hf2d
