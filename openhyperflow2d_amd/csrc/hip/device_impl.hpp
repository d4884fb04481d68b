// Internals of DeviceSolver shared by the solver's translation units (a few
// .hip units by kernel family, see device_solver.hip): error checks, the device
// allocator, DeviceSolver::Impl and the step-graph cache.  Included by those
// .hip files only; it defines no kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <rocprofiler-sdk-roctx/roctx.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../core/flow_stats.hpp"
#include "../core/lean_euler.hpp"
#include "../core/solver.hpp"
#include "device_solver.hpp"
#include "dev_common.hpp"
#include "chem_fast.hpp"
#include "chem_rtc.hpp"
#include "chem_mech.hpp"
#include "solver_args.hpp"

#define HIP_CHECK(x)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (x);                                                                         \
    if (e_ != hipSuccess)                                                                        \
      throw std::runtime_error(std::string("HIP error ") + hipGetErrorString(e_) + " at " +      \
                               __FILE__ + ":" + std::to_string(__LINE__));                       \
  } while (0)
#define NCCL_CHECK(x)                                                                            \
  do {                                                                                           \
    ncclResult_t r_ = (x);                                                                       \
    if (r_ != ncclSuccess)                                                                       \
      throw std::runtime_error(std::string("RCCL error ") + ncclGetErrorString(r_) + " at " +    \
                               __FILE__ + ":" + std::to_string(__LINE__));                       \
  } while (0)

namespace hf2d {

struct DevBuf {
  std::vector<void*> ptrs;
  template <class T>
  T* alloc(size_t n) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    HIP_CHECK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T)));
    ptrs.push_back(p);
    return (T*)p;
  }
  ~DevBuf() {
    for (void* p : ptrs) (void)hipFree(p);
  }
};

// A device array that only grows: arming a recorder again, or a plan rebuilt
// by upload(), uses what is there while it fits, so doing either over and over
// does not grow device memory.  n == 0 allocates nothing.
template <class T>
struct DevArray {
  T* p = nullptr;
  size_t cap = 0;
  // true: allocated (zero-filled by memsets of the null stream: synchronise before the solver stream uses it)
  bool ensure(DevBuf& mem, size_t n) {
    if (n <= cap) return false;
    p = mem.alloc<T>(n);
    cap = n;
    return true;
  }
};

struct DeviceSolver::Impl {
  DevBuf mem;
  hipStream_t stream = nullptr;
  // comm overlap: the halo of the edge tiles travels on comm_stream while the
  // interior tiles compute on `stream` (events ev_edge / ev_halo join them)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_edge = nullptr, ev_halo = nullptr;
  // device arrays (same roles as HostArrays)
  real *S[2], *A[2], *B[2], *F, *Src, *SrcAdd, *beta, *dSdx[2], *dSdy[2];
  real *U[2], *V[2], *Tg[2], *p, *kk, *R, *CP, *lam, *mu, *mu_t, *lam_t, *Diff, *Y;
  real *l_min, *y_plus, *Re_local, *BGX, *BGY, *Tf, *Q_conv, *grad, *qdir;
  u64 *CT, *TT;
  uint8_t* nb;
  // lean inviscid state: pre-chemistry species and pressure (ping-pong with
  // U/V on pbuf), per-cell neighbour/publish byte
  real *Spre[2], *P2[2];
  // lean N-S: second level of CP / mu / lam / k (the first is the generic array)
  real *CP2 = nullptr, *mu2 = nullptr, *lam2 = nullptr, *kk2 = nullptr, *mu_t2 = nullptr;
  // lean mechanism step: second level of p and both levels of the stored T
  // (the thermodynamic state T, p, Cp, k of lean_mech.hpp; Cp / k share CP2 / kk2)
  real *p2 = nullptr, *Tst[2] = {nullptr, nullptr};
  // both levels of every two-level array, [0] the generic one (cbuf indexes them)
  struct Levels {
    real *CP[2], *mu[2], *lam[2], *kk[2], *mu_t[2], *p[2];
  };
  Levels levels() const { return {{CP, CP2}, {mu, mu2}, {lam, lam2}, {kk, kk2}, {mu_t, mu_t2}, {p, p2}}; }
  void alloc_levels(long N) {   // (the lean N-S and the lean mechanism step share them)
    if (CP2) return;
    CP2 = mem.alloc<real>(N);
    mu2 = mem.alloc<real>(N);
    lam2 = mem.alloc<real>(N);
    kk2 = mem.alloc<real>(N);
    mu_t2 = mem.alloc<real>(N);
  }
  unsigned long long* lnm_trace = nullptr;   // HF2D_LNM_TRACE phase clocks
  long lnm_trace_n = 0;
  uint8_t* lb;
  uint8_t* gf;   // generic-stepper GF_* traffic flags
  int32_t* wslot;
  // K10 (y+): owned wall nodes, their friction velocities, all strips' values
  long* wall_own = nullptr;
  real *wall_uw = nullptr, *uw_all = nullptr;
  uint8_t *wall_ok = nullptr, *uw_all_ok = nullptr;
  // mechanism mode (SK_MECH): species block, Ys ping-pongs with S (sbuf)
  MechData* mech = nullptr;
  int nsp = 0;
  std::unique_ptr<ChemMechPack> chem_pack;   // MFMA kinetics kernel's mechanism image
  int* chem_list = nullptr;                  // compacted kinetics: reacting cells of the step
  unsigned* chem_count = nullptr;
  real *Ys[2] = {nullptr, nullptr}, *As = nullptr, *Bs = nullptr, *Fs = nullptr, *betas = nullptr;
  real *dSdxs[2] = {nullptr, nullptr}, *dSdys[2] = {nullptr, nullptr};
  SpeciesProps* species = nullptr;   // (the sp of a SpeciesDev: air_table_of)
  SpeciesDev species_host;           // what upload() copied there
  ScenarioTables* scen = nullptr;
  long* probe_idx = nullptr;   // K8 monitor probes (sample_monitors)
  real* probe_out = nullptr;
  // The recorders: the argument block the kernels take, and behind it the
  // arrays its pointers are set from (DevArray: arming again reuses what fits)
  ProbeRing ring{};            // per-step recorder (record_probes); cap == 0: not armed
  struct {
    DevArray<long> idx;
    DevArray<real> rows;
    DevArray<double> times;
    DevArray<unsigned long long> count;
  } ring_mem;
  LoadsDev loads{};            // per-step load recorder (record_loads); cap == 0: not armed
  struct {
    DevArray<long> cell, cell2, off;
    DevArray<real> coef, scratch, vals;
    DevArray<uint8_t> kind;
    DevArray<double> times;
    DevArray<unsigned long long> count;
  } loads_mem;
  struct SampleRingMem {   // the arrays behind a SampleRing
    DevArray<real> vals;
    DevArray<double> times, stat;
    DevArray<WallHeatScalars> sc;
  };
  // A recorder's array of n entries, and a plan's host vector in one, while the
  // stream is idle (the caller waits for the copies before the vector goes).
  template <class T>
  T* grown(DevArray<T>& a, size_t n) {
    if (a.ensure(mem, n)) HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
    return a.p;
  }
  template <class T>
  const T* plan_array(DevArray<T>& a, const std::vector<T>& v) {
    grown(a, v.size());
    if (!v.empty()) HIP_CHECK(hipMemcpyAsync(a.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
    return a.p;
  }
  // The sampled ring of the wall heat and the surface recorder: arrays for
  // `cap` rows of `ne` entries behind r; ring and statistics empty with the
  // clock at now (t_off: the solver's time_offset); both read back to the host
  // (the last two in observe.hip, beside the kernels).
  void ring_alloc(SampleRingMem& a, SampleRing& r, size_t ne, int cap) {
    r.vals = grown(a.vals, (size_t)cap * ne);
    r.times = grown(a.times, (size_t)cap);
    r.stat = grown(a.stat, 4 * ne);
    r.sc = grown(a.sc, 1);
    r.cap = cap;
  }
  void ring_reset(const SampleRing& r, size_t ne, int every, bool step_weight, double t_off);
  SampledRing ring_read(const SampleRing& r, size_t ne);
  WallHeatDev wallq{};         // per-step wall heat recorder (record_wall_heat)
  struct {
    DevArray<long> cells;
    DevArray<int> node5, off, list;
    DevArray<real> scratch;
    SampleRingMem ring;
  } wallq_mem;
  SurfaceDev surf{};           // per-step surface recorder (record_surface)
  struct {
    DevArray<long> cells;
    DevArray<uint8_t> mask, bits;
    DevArray<int> idx;
    DevArray<real> scratch;
    SampleRingMem ring;
  } surf_mem;
  FrameDev frames{};           // per-step frame recorder (record_frames)
  struct {
    DevArray<real> scratch;
    SampleRingMem ring;          // (stat stays empty: the frames keep no statistics)
  } frames_mem;
  FlowStats stats{};           // whole-field statistics (start_averaging)
  size_t stats_planes = 0;     // planes of N doubles allocated behind stats.m
  size_t stats_used = 0;       // of which the armed options use (stats_plane_count)
  StatsExt stats_x{};          // species list and the favre / species planes inside them
  DevScalars* sc = nullptr;
  DevScalars* sc_host = nullptr;   // pinned
  // single GPU: the last (output) lean tile step of a host call wrote the
  // scalars into sc_host itself (DeviceSolver::host_tail); sync_scalars then
  // only waits
  bool sc_mirrored = false;
  unsigned* host_done = nullptr;   // host_tail's completion counters
  hipEvent_t lnm_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // DeviceSolver::lnm_timing
  FusedX* fx_dev = nullptr;   // fx_device: the tile kernels' copy of fused_args()
  FusedX fx_dev_host{};
  bool fx_dev_valid = false;
  // fused lean N-S / mechanism steps: the HALO_LNS list of the last fused
  // step, whose halo is still in the mailbox (lns_ghost_pending), and device
  // copies of the lists of both buffer parities (the next step's prologue)
  ColList lns_pend{};
  ColList* lc_dev = nullptr;
  ColList lc_host[2]{};
  bool lc_valid[2] = {false, false};
  int lc_next = 0;
  ResidualPack* partials = nullptr;
  ResidualPack* res_out = nullptr;
  ResidualPack* res_host = nullptr;   // pinned
  long max_partials = 0;
  real* halo_send[2] = {nullptr, nullptr};
  real* halo_recv[2] = {nullptr, nullptr};
  long halo_cap = 0;
  double* dt_recv = nullptr;   // dt of every rank (gathered with the halo)
  ncclComm_t comm = nullptr;
  std::shared_ptr<LocalGroup> local;   // in-process virtual ranks (testing)
  int rank = 0, nranks = 1;
  // xGMI peer-to-peer transport (hf2d_p2p_xchg)
  struct P2P {
    bool on = false;
    char* base = nullptr;                 // fine-grained mailbox (p2p_layout)
    size_t bytes = 0, off_dtr = 0, off_recv = 0;
    unsigned long long* seq = nullptr;    // device-side exchange counter
    unsigned* done = nullptr;             // fused tile kernel: finished workgroups
    std::vector<char*> peer_base;         // mailbox of every rank (self: base)
    std::vector<void*> opened;            // IPC mappings to close
    unsigned long long** d_flags = nullptr;
    double** d_dtr = nullptr;
    bool loop = false;                    // p2p_loopback: the neighbours' mailboxes are this rank's own
    // mailbox the edge pushes of `side` land in (0: the left neighbour's,
    // whose right side this rank is); loopback: this rank's own mailbox of
    // that side, so the ghost columns take the strip's own edge values
    real* push_base(int side, int rank, long cap) const {
      if (loop) return (real*)(base + off_recv) + (side == 0 ? -cap : cap);
      return (real*)(peer_base[side == 0 ? rank - 1 : rank + 1] + off_recv);
    }
  } p2p;

  LeanSoA lean_view(const HostArrays& h, int sb, int ab, int db, int pb, bool fromg) const {
    LeanSoA L;
    L.N = h.N;
    L.Sin = S[sb];
    L.Sout = S[1 - sb];
    L.Pin_s = Spre[pb];
    L.Pout_s = Spre[1 - pb];
    L.beta = beta;
    L.Uin = U[pb];
    L.Vin = V[pb];
    L.Pin = fromg ? p : P2[pb];
    L.Uout = U[1 - pb];
    L.Vout = V[1 - pb];
    L.Pout = P2[1 - pb];
    L.Tout = Tg[1 - pb];
    L.dSdx_in = dSdx[db];
    L.dSdy_in = dSdy[db];
    L.dSdx_out = dSdx[1 - db];
    L.dSdy_out = dSdy[1 - db];
    L.CT = CT;
    L.lb = lb;
    L.CP = CP;
    L.R = R;
    L.kk = kk;
    L.Y = Y;
    L.Tf = Tf;
    L.BGX = BGX;
    L.BGY = BGY;
    L.SrcAdd = SrcAdd;
    L.gA = A[ab];
    L.gB = B[ab];
    L.gF = F;
    return L;
  }

  // lean N-S kernel arguments: Sp^m in S[1-sb], level m-1 primitives in
  // U/V/Tg[1-pb] and CPx[1-cb]; K_m writes Sp^{m+1} into S[sb], level m into
  // U/V/Tg[pb] and CPx[cb] (CPx[0] = the generic arrays)
  LnsArrays lns_arrays(const HostArrays& h, int sb, int pb, int cb, int db, int ab) const {
    LnsArrays a;
    a.N = h.N;
    a.Sp = S[1 - sb];
    a.Sp_out = S[sb];
    a.beta = beta;
    a.Ui = U[1 - pb];
    a.Vi = V[1 - pb];
    a.Ti = Tg[1 - pb];
    a.Uo = U[pb];
    a.Vo = V[pb];
    a.To = Tg[pb];
    const Levels x = levels();
    a.CPi = x.CP[1 - cb];
    a.mui = x.mu[1 - cb];
    a.lami = x.lam[1 - cb];
    a.kki = x.kk[1 - cb];
    a.CPo = x.CP[cb];
    a.muo = x.mu[cb];
    a.lamo = x.lam[cb];
    a.kko = x.kk[cb];
    a.mu_ti = x.mu_t[1 - cb];
    a.mu_to = x.mu_t[cb];
    a.l_min = l_min;
    a.y_plus = y_plus;
    a.Src = Src;
    a.gA = A[ab];
    a.gB = B[ab];
    a.gF = F;
    a.R = R;
    a.BGX = BGX;
    a.BGY = BGY;
    a.grad = grad;
    a.SrcAdd = SrcAdd;
    a.dSdx_in = dSdx[db];
    a.dSdy_in = dSdy[db];
    a.dSdx_out = dSdx[1 - db];
    a.dSdy_out = dSdy[1 - db];
    a.CT = CT;
    a.TT = TT;
    a.nb = nb;
    a.gf = gf;
    return a;
  }

  // lean mechanism step arguments (lean_mech.hpp): Sp^m in S[1-sb], its
  // post-kinetics species in Ys[sb]; every two-level array is read at
  // [1 - cb] and written at [cb] (transport m-1 -> m, state m -> m+1)
  LnmArrays lnm_arrays(const HostArrays& h, int sb, int pb, int cb, int db, int ab) const {
    LnmArrays a;
    a.N = h.N;
    a.mech = mech;
    a.nsp = nsp;
    a.bath = h.mech ? h.mech->bath : 0;
    a.Sp = S[1 - sb];
    a.Sp_out = S[sb];
    a.Ys = Ys[sb];
    a.Ys_out = Ys[1 - sb];
    a.beta = beta;
    a.betas = betas;
    a.Ui = U[1 - pb];
    a.Vi = V[1 - pb];
    a.Ti = Tg[1 - pb];
    a.Uo = U[pb];
    a.Vo = V[pb];
    a.To = Tg[pb];
    const Levels x = levels();
    a.mui = x.mu[1 - cb];
    a.lami = x.lam[1 - cb];
    a.mu_ti = x.mu_t[1 - cb];
    a.muo = x.mu[cb];
    a.lamo = x.lam[cb];
    a.mu_to = x.mu_t[cb];
    a.Tsi = Tst[1 - cb];
    a.psi = x.p[1 - cb];
    a.CPsi = x.CP[1 - cb];
    a.ksi = x.kk[1 - cb];
    a.Tso = Tst[cb];
    a.pso = x.p[cb];
    a.CPso = x.CP[cb];
    a.kso = x.kk[cb];
    a.l_min = l_min;
    a.y_plus = y_plus;
    a.BGX = BGX;
    a.BGY = BGY;
    a.grad = grad;
    a.Src = Src;
    a.SrcAdd = SrcAdd;
    a.gA = A[ab];
    a.gB = B[ab];
    a.gF = F;
    a.dSdx_in = dSdx[db];
    a.dSdy_in = dSdy[db];
    a.dSdx_out = dSdx[1 - db];
    a.dSdy_out = dSdy[1 - db];
    a.dSdxs_in = dSdxs[db];
    a.dSdys_in = dSdys[db];
    a.dSdxs_out = dSdxs[1 - db];
    a.dSdys_out = dSdys[1 - db];
    a.CT = CT;
    a.TT = TT;
    a.nb = nb;
    a.gf = gf;
    a.hot = chem_list;
    return a;
  }

  SoA view(const HostArrays& h, int sb, int ab, int db, int pb) const {
    SoA s;
    s.nx = h.nx;
    s.ny = h.ny;
    s.N = h.N;
    s.S = S[sb];
    s.A = A[ab];
    s.B = B[ab];
    s.F = F;
    s.Src = Src;
    s.SrcAdd = SrcAdd;
    s.beta = beta;
    s.dSdx = dSdx[db];
    s.dSdy = dSdy[db];
    s.U = U[pb];
    s.V = V[pb];
    s.Tg = Tg[pb];
    s.p = p;
    s.kk = kk;
    s.R = R;
    s.CP = CP;
    s.lam = lam;
    s.mu = mu;
    s.mu_t = mu_t;
    s.lam_t = lam_t;
    s.Diff = Diff;
    s.Y = Y;
    s.l_min = l_min;
    s.y_plus = y_plus;
    s.Re_local = Re_local;
    s.BGX = BGX;
    s.BGY = BGY;
    s.Tf = Tf;
    s.Q_conv = Q_conv;
    s.grad = grad;
    s.CT = CT;
    s.TT = TT;
    s.nb = nb;
    s.gf = gf;
    s.wslot = wslot;
    mech_view(s, sb, db);
    return s;
  }
  void mech_view(SoA& s, int yb, int db) const {
    s.mech = mech;
    s.nsp = nsp;
    if (!mech) return;
    s.Ys = Ys[yb];
    s.As = As;
    s.Bs = Bs;
    s.Fs = Fs;
    s.betas = betas;
    s.dSdxs = dSdxs[db];
    s.dSdys = dSdys[db];
  }

  // on_cycle_roll: the device's time_part restarts T lower, and every stored
  // value of it moves with it: the n entries of a device array (none: nothing to do)
  void shift_times(double* a, size_t n, double T) {
    if (!n) return;
    std::vector<double> t(n);
    HIP_CHECK(hipMemcpyAsync(t.data(), a, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    for (double& x : t) x -= T;
    HIP_CHECK(hipMemcpyAsync(a, t.data(), n * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
  }
  // ... the offset of a tick's clock, time_part - t_off, which so goes on unbroken
  void shift_clock(StatsScalars* sc, double T) { shift_times(&sc->t_off, 1, T); }
  // ... and a sampled ring: its rows' times and its peak times (all set once a sample was taken)
  void shift_ring(const SampleRing& r, size_t ne, double T) {
    shift_times(r.times, (size_t)r.cap, T);
    shift_times(r.stat + 3 * ne, ne, T);
  }
};

struct DeviceSolver::GraphCache {
  hipGraphExec_t exec = nullptr;
  uint64_t sig = 0;
  // fused lean N-S windows: the first step unpacks the previous step's halo
  // in its prologue (needs the mailbox to hold an lns list's publication at
  // replay), and the window ends with its last step's halo pending
  bool lns_pro = false, lns_end = false;
  ColList lns_end_list{};
  DeviceSolver::TileLast tile_last;   // lean_tile_last of the window's last step
  ~GraphCache() {
    if (exec) (void)hipGraphExecDestroy(exec);
  }
};

}  // namespace hf2d
