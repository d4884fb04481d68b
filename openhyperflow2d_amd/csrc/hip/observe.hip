// Observers of the run: monitor points, the per-step probe recorder
// (probe_history.hpp), the per-step load recorder (load_history.hpp), the
// per-step wall heat recorder (wall_heat.hpp), the per-step surface recorder
// (surface_history.hpp) and the time-averaged flow statistics (flow_stats.hpp).

#include "device_impl.hpp"
#include "flow_stats.hpp"
#include "load_history.hpp"
#include "wall_heat.hpp"
#include "surface_history.hpp"

namespace hf2d {

// K8 monitors: p and Tg of the probe cells this rank owns (idx < 0: not
// owned) gathered on the device, so an output step moves 16 bytes per probe
// instead of the whole state.
__global__ void hf2d_probe_gather(const long* idx, int n, const real* p, const real* T, real* out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const long c = idx[t];
  out[2 * t] = c >= 0 ? p[c] : 0.0;
  out[2 * t + 1] = c >= 0 ? T[c] : 0.0;
}

void DeviceSolver::sample_monitors(std::vector<MonitorPoint>& mp) {
  if (mp.empty()) return;
  flush_pending();
  p2p_complete();
  Impl& m = *impl;
  if (lns_state) lns_materialize();
  const int n = (int)mp.size();
  std::vector<long> idx(n, -1);
  for (int q = 0; q < n; q++) {
    const int i = (int)(mp[q].x / cs.cfg.dx), j = (int)(mp[q].y / cs.cfg.dy);
    if (cs.J.in(i, j) && i >= gi0 && i < gi1) idx[q] = (long)(i - gi0 + l_off) * h.ny + j;
  }
  if ((int)probe_idx_host.size() != n) {
    probe_idx_host.assign(n, -2);
    probe_buf_host.assign(2 * n, 0.0);
    impl->probe_idx = m.mem.alloc<long>(n);
    impl->probe_out = m.mem.alloc<real>(2 * n);
    HIP_CHECK(hipDeviceSynchronize());
  }
  if (idx != probe_idx_host) {
    probe_idx_host = idx;
    HIP_CHECK(hipMemcpyAsync(m.probe_idx, probe_idx_host.data(), n * sizeof(long), hipMemcpyHostToDevice, m.stream));
  }
  // current pressure: the lean arrays while they are authoritative
  const real* p = lean_state ? m.P2[pbuf] : m.p;
  hipLaunchKernelGGL(hf2d_probe_gather, dim3((n + 63) / 64), dim3(64), 0, m.stream, m.probe_idx, n, p, m.Tg[pbuf],
                     m.probe_out);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(probe_buf_host.data(), m.probe_out, 2 * n * sizeof(real), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  for (int q = 0; q < n; q++) {
    real pv = probe_buf_host[2 * q], Tv = probe_buf_host[2 * q + 1];
    const int i = (int)(mp[q].x / cs.cfg.dx), j = (int)(mp[q].y / cs.cfg.dy);
    if (comm->size() > 1) {   // exactly one rank owns the probe
      pv = comm->allreduce_sum(pv);
      Tv = comm->allreduce_sum(Tv);
    } else if (!cs.J.in(i, j)) {
      continue;
    }
    mp[q].p = pv;
    mp[q].T = Tv;
  }
}

// ---------------------------------------------------------------------------
// Per-step probe recorder (hip/probe_history.hpp)
// ---------------------------------------------------------------------------
void DeviceSolver::record_probes(const std::vector<std::pair<int, int>>& cells, long capacity) {
  check_probe_cells(cells, capacity);
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const int n = (int)cells.size();
  probe_rec_idx.assign(n, -1);
  for (int q = 0; q < n; q++) {
    const int i = cells[q].first, j = cells[q].second;
    if (i < gi0 || i >= gi1) continue;   // another strip's column
    const long c = (long)(i - gi0 + l_off) * h.ny + j;
    // (a trimmed strip rank's Case could not check its flags in check_probe_cells)
    if (has_all(h.CT[c], CT_SOLID) || !has_all(h.CT[c], CT_NODE_IS_SET))
      throw std::invalid_argument("record_probes: cell (" + std::to_string(i) + ", " + std::to_string(j) +
                                  ") is solid or not set");
    probe_rec_idx[q] = c;
  }
  // (outside any capture: flush_pending ran the queued steps, and a capture
  // only lives inside run_graph)
  ProbeRing r;
  r.n = n;
  r.cap = (int)std::min<long>(capacity, 0x7fffffffL);
  long* idx = m.mem.alloc<long>(n);
  r.idx = idx;
  r.rows = m.mem.alloc<real>((size_t)r.cap * n * PROBE_VARS);
  r.times = m.mem.alloc<double>((size_t)r.cap);
  r.count = m.mem.alloc<unsigned long long>(1);
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
  HIP_CHECK(hipMemcpyAsync(idx, probe_rec_idx.data(), n * sizeof(long), hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  m.ring = r;
  probe_cap = r.cap;
  probe_gen++;   // windows captured so far must not replay (mode_signature)
}

void DeviceSolver::clear_probe_history() {
  if (!probe_cap) return;
  flush_pending();
  Impl& m = *impl;
  HIP_CHECK(hipMemsetAsync(m.ring.count, 0, sizeof(unsigned long long), m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

ProbeHistory DeviceSolver::probe_history() {
  if (!probe_cap) throw std::runtime_error("probe_history: no recorder armed (record_probes)");
  flush_pending();
  Impl& m = *impl;
  const ProbeRing& r = m.ring;
  const size_t row = (size_t)r.n * PROBE_VARS;
  unsigned long long total = 0;
  std::vector<real> rows((size_t)r.cap * row);
  std::vector<double> tp((size_t)r.cap);
  HIP_CHECK(hipMemcpyAsync(&total, r.count, sizeof total, hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipMemcpyAsync(rows.data(), r.rows, rows.size() * sizeof(real), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipMemcpyAsync(tp.data(), r.times, tp.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  ProbeHistory H;
  H.nprobes = r.n;
  H.total = (long)total;
  const long cap = r.cap, n = std::min<long>(H.total, cap), first = H.total > cap ? H.total % cap : 0;
  H.times.resize(n);
  H.values.resize((size_t)n * row);
  for (long k = 0; k < n; k++) {
    const long s = (first + k) % cap;
    // the device accumulates time since the cycle start (on_cycle_roll moved
    // the rows of earlier cycles with it); the host's time is
    // global_time + (time_part - time_offset) (sync_scalars, summary)
    const real part = tp[s] - time_offset;
    H.times[k] = cs.global_time + part;
    std::copy(rows.begin() + s * row, rows.begin() + (s + 1) * row, H.values.begin() + k * row);
  }
  H.owned.resize(r.n);
  for (int q = 0; q < r.n; q++) H.owned[q] = probe_rec_idx[q] >= 0 ? 1 : 0;
  return H;
}

// Last launch of a step: the row of every probe from the post-step buffers,
// in the representation that is authoritative now (the views download() /
// lns_materialize() would read).
int DeviceSolver::post_step_view(SoA& s) const {
  const Impl& m = *impl;
  int kind = PR_GATHER;
  if (lns_state) {
    // lean N-S / mechanism: Sp^{m+1} and the lagged level (lns_materialize's input view)
    s = m.view(h, 1 - sbuf, abuf, dsbuf, 1 - pbuf);
    const Impl::Levels x = m.levels();
    if (m.mech) {
      kind = PR_MECH;
      s.kk = x.kk[cbuf];         // the lagged k of fill_node's skip test
      s.Tg = m.Tst[1 - cbuf];    // stored state of the new level
      s.p = x.p[1 - cbuf];
      // the post-kinetics species of Sp^{m+1} (lnm_arrays: Ys[sb] beside
      // S[1 - sb]), which lns_materialize leaves where they are and download()
      // reads; the other paths' view holds Ys[sbuf] already
      s.Ys = m.Ys[sbuf];
    } else {
      kind = sk_mode == SK_SGT ? PR_SGT : PR_SGL;
      s.CP = x.CP[1 - cbuf];
      s.mu = x.mu[1 - cbuf];
      s.lam = x.lam[1 - cbuf];
      s.kk = x.kk[1 - cbuf];
      s.mu_t = x.mu_t[1 - cbuf];
    }
  } else {
    s = m.view(h, sbuf, abuf, dsbuf, pbuf);
    if (lean_state) {
      s.p = m.P2[pbuf];
      if (!lean_T_stored) kind = PR_LEAN;
    }
  }
  return kind;
}

void DeviceSolver::launch_probe_record(const StepParams& P) {
  Impl& m = *impl;
  SoA s;
  const int kind = post_step_view(s);
  const dim3 g(1), b(PROBE_MAX);
  switch (kind) {
    case PR_SGL: hipLaunchKernelGGL(hf2d_probe_record<PR_SGL>, g, b, 0, m.stream, P, s, m.ring, m.sc); break;
    case PR_SGT: hipLaunchKernelGGL(hf2d_probe_record<PR_SGT>, g, b, 0, m.stream, P, s, m.ring, m.sc); break;
    case PR_MECH: hipLaunchKernelGGL(hf2d_probe_record<PR_MECH>, g, b, 0, m.stream, P, s, m.ring, m.sc); break;
    case PR_LEAN: hipLaunchKernelGGL(hf2d_probe_record<PR_LEAN>, g, b, 0, m.stream, P, s, m.ring, m.sc); break;
    default: hipLaunchKernelGGL(hf2d_probe_record<PR_GATHER>, g, b, 0, m.stream, P, s, m.ring, m.sc); break;
  }
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Per-step load recorder (hip/load_history.hpp)
// ---------------------------------------------------------------------------
void DeviceSolver::record_loads(const std::vector<LoadBox>& boxes, const std::vector<LoadCut>& cuts, long capacity) {
  check_record_loads(boxes, cuts, capacity);   // (the arguments; one strip of several refuses)
  Impl& m = *impl;
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  // (a refused plan throws here and leaves the armed recorder, if any, whole:
  // its boxes, cuts, plan and ring are replaced only together, below)
  LoadPlan P = loads_plan_build(boxes, cuts);
  const int cap = (int)std::min<long>(capacity, 0x7fffffffL);
  const size_t nv = (size_t)cap * P.nlists();
  LoadsDev& L = m.loads;
  // (arrays that are large enough are used again: arming over and over does not grow device memory)
  if (nv > m.loads_vals_cap) {
    m.loads_vals = m.mem.alloc<real>(nv);
    m.loads_vals_cap = nv;
  }
  if ((size_t)cap > m.loads_times_cap) {
    m.loads_times = m.mem.alloc<double>((size_t)cap);
    m.loads_times_cap = (size_t)cap;
  }
  if (!L.count) L.count = m.mem.alloc<unsigned long long>(1);
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
  loads_cap = 0;
  loads_plan_upload(std::move(P));
  loads_boxes = boxes;
  loads_cuts = cuts;
  L.vals = m.loads_vals;
  L.times = m.loads_times;
  L.cap = cap;
  HIP_CHECK(hipMemsetAsync(L.count, 0, sizeof(unsigned long long), m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  loads_cap = cap;
}

// The plan of the boxes and cuts over the records the backend holds now.
// Throws where a term could not be evaluated exactly.
LoadPlan DeviceSolver::loads_plan_build(const std::vector<LoadBox>& boxes, const std::vector<LoadCut>& cuts) const {
  LoadPlan P = build_load_plan(cs, cs.J, boxes, cuts, l_off);
  for (long c : P.cell)
    if (c < 0 || c >= h.N) throw std::runtime_error("load recorder: a term's cell lies outside the solver's arrays");
  for (long c : P.cell2)
    if (c < 0 || c >= h.N) throw std::runtime_error("load recorder: a term's cell lies outside the solver's arrays");
  // the lean N-S / mechanism kinds fill a wall node with the parameters of the
  // recorded step; the fill a download runs takes the next step's, whose
  // is_mu_t differs after the last step before TurbStartIter.  That step is a
  // lean one only where the steps before it are (lns_step_ok: no is_init, the
  // same is_mu_t as the step before).  lns_ok / lnm_ok are what upload() found
  // eligible, whatever the lean_ns / lean_mech switches say now or later, and
  // an iteration count at or past TurbStartIter stays there, so the answer
  // holds for every later step; upload() asks again for the plan it rebuilds.
  // (the lean mechanism state exists for at most LNM_NSB = 9 species, the
  // block loads_wall_fill runs the fill with: lnm_ok)
  const bool box_terms = P.off[(size_t)LOAD_PARTS * P.nboxes] > 0;
  if (box_terms && (lns_ok || lnm_ok) && cs.cfg.ProblemType == SM_NS && !cs.cfg.isTurbulenceReset &&
      cs.cfg.TurbStartIter >= 2 && last_iter + iter < (long)cs.cfg.TurbStartIter)
    throw std::runtime_error("load recorder: wall terms on the lean N-S / mechanism state cannot be recorded exactly "
                             "before TurbStartIter has passed; arm (or upload) later");
  return P;
}

// A built plan into the device arrays (used again where they are large
// enough; the stream is idle: flush_pending / upload synchronised it).
void DeviceSolver::loads_plan_upload(LoadPlan&& P) {
  Impl& m = *impl;
  const long nt = P.nterms();
  const int nl = P.nlists();
  if (nt > m.loads_terms_cap) {
    m.loads_cell = m.mem.alloc<long>((size_t)nt);
    m.loads_cell2 = m.mem.alloc<long>((size_t)nt);
    m.loads_coef = m.mem.alloc<real>((size_t)nt);
    m.loads_kind = m.mem.alloc<uint8_t>((size_t)nt);
    m.loads_scratch = m.mem.alloc<real>((size_t)nt);
    m.loads_terms_cap = nt;
  }
  if (nl + 1 > m.loads_off_cap) {
    m.loads_off = m.mem.alloc<long>((size_t)nl + 1);
    m.loads_off_cap = nl + 1;
  }
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets, and nothing in flight reads the arrays)
  auto cp = [&](void* d, const void* s, size_t bytes) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, m.stream));
  };
  cp(m.loads_cell, P.cell.data(), nt * sizeof(long));
  cp(m.loads_cell2, P.cell2.data(), nt * sizeof(long));
  cp(m.loads_coef, P.coef.data(), nt * sizeof(real));
  cp(m.loads_kind, P.kind.data(), nt * sizeof(uint8_t));
  cp(m.loads_off, P.off.data(), ((size_t)nl + 1) * sizeof(long));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  LoadsDev& L = m.loads;
  L.cell = m.loads_cell;
  L.cell2 = m.loads_cell2;
  L.coef = m.loads_coef;
  L.kind = m.loads_kind;
  L.off = m.loads_off;
  L.scratch = m.loads_scratch;
  L.nterms = nt;
  L.nlists = nl;
  loads_plan = std::move(P);
  loads_friction = loads_plan.friction();
  loads_gen++;   // windows captured so far must not replay (mode_signature)
}

// upload() replaced the records under an armed recorder: the same boxes and
// cuts over the new flags (as many lists as before: the ring keeps its shape).
void DeviceSolver::loads_plan_rebuild() { loads_plan_upload(loads_plan_build(loads_boxes, loads_cuts)); }

void DeviceSolver::clear_load_history() {
  if (!loads_cap) return;
  flush_pending();
  Impl& m = *impl;
  HIP_CHECK(hipMemsetAsync(m.loads.count, 0, sizeof(unsigned long long), m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

LoadHistory DeviceSolver::load_history() {
  if (!loads_cap) throw std::runtime_error("load_history: no recorder armed (record_loads)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const LoadsDev& L = m.loads;
  unsigned long long total = 0;
  std::vector<real> vals((size_t)L.cap * L.nlists);
  std::vector<double> tp((size_t)L.cap);
  HIP_CHECK(hipMemcpyAsync(&total, L.count, sizeof total, hipMemcpyDeviceToHost, m.stream));
  if (!vals.empty())
    HIP_CHECK(hipMemcpyAsync(vals.data(), L.vals, vals.size() * sizeof(real), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipMemcpyAsync(tp.data(), L.times, tp.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  // (the probe ring's clock: probe_history)
  return load_history_from_ring(loads_plan, vals.data(), (long)total, (long)L.cap, [&](long s) {
    const real part = tp[s] - time_offset;
    return (double)(cs.global_time + part);
  });
}

// The views the fill of lns_materialize would run over now (its sin == pold
// and its out), without running it.
void DeviceSolver::lns_fill_views(SoA& sin, SoA& out) const {
  const Impl& m = *impl;
  const Impl::Levels x = m.levels();
  sin = m.view(h, 1 - sbuf, abuf, dsbuf, 1 - pbuf);
  if (m.mech) {
    m.mech_view(sin, sbuf, dsbuf);
    sin.mu = x.mu[1 - cbuf];
    sin.lam = x.lam[1 - cbuf];
    sin.mu_t = x.mu_t[1 - cbuf];
    sin.CP = x.CP[cbuf];
    sin.kk = x.kk[cbuf];
    sin.p = x.p[cbuf];
  } else {
    sin.CP = x.CP[1 - cbuf];
    sin.mu = x.mu[1 - cbuf];
    sin.lam = x.lam[1 - cbuf];
    sin.kk = x.kk[1 - cbuf];
    sin.mu_t = x.mu_t[1 - cbuf];
  }
  out = m.view(h, sbuf, abuf, dsbuf, pbuf);
}

// After the other observers' launches; the same view, and for the lean N-S /
// mechanism state the materialise fill's.  Nothing here allocates, copies or
// synchronises.
void DeviceSolver::launch_loads(const StepParams& P, int slot, int slot_next) {
  Impl& m = *impl;
  SoA s;
  const int kind = post_step_view(s);
  SoA fin = s, out = s;
  // the dt slot of lns_materialize's fill, which runs after nstep++ (SGL: nstep % 3, else (nstep + 2) % 3)
  int fslot = slot;
  if (lns_state) {
    lns_fill_views(fin, out);
    if (kind == PR_SGL) fslot = slot_next;
  }
  const LoadsDev& L = m.loads;
  if (L.nterms > 0) {
    const dim3 g((unsigned)((L.nterms + LOADS_BLOCK - 1) / LOADS_BLOCK)), b(LOADS_BLOCK);
    switch (kind) {
      case PR_SGL: hipLaunchKernelGGL(hf2d_loads_terms<PR_SGL>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_SGT: hipLaunchKernelGGL(hf2d_loads_terms<PR_SGT>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_MECH: hipLaunchKernelGGL(hf2d_loads_terms<PR_MECH>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      default: hipLaunchKernelGGL(hf2d_loads_terms<PR_GATHER>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
    }
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(hf2d_loads_fold, dim3(1), dim3(LOADS_FOLD_WAVES * WAVE), 0, m.stream, L, m.sc);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Per-step wall heat recorder (hip/wall_heat.hpp)
// ---------------------------------------------------------------------------
void DeviceSolver::record_wall_heat(const WallHeatOpts& o) {
  check_record_wall_heat(o);   // (the options; one strip of several refuses)
  Impl& m = *impl;
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  // (a refused plan throws here and leaves the armed recorder, if any, whole:
  // its options, plan, ring and statistics are replaced only together, below)
  WallHeatPlan P = wallq_plan_build(o);
  const int cap = (int)std::min<long>(o.capacity, 0x7fffffffL);
  const size_t ne = (size_t)P.nentries(), nv = (size_t)cap * ne;
  WallHeatDev& L = m.wallq;
  // (arrays that are large enough are used again: arming over and over does not grow device memory)
  if (nv > m.wallq_vals_cap) {
    m.wallq_vals = m.mem.alloc<real>(nv);
    m.wallq_vals_cap = nv;
  }
  if ((size_t)cap > m.wallq_times_cap) {
    m.wallq_times = m.mem.alloc<double>((size_t)cap);
    m.wallq_times_cap = (size_t)cap;
  }
  if (!m.wallq_stat) m.wallq_stat = m.mem.alloc<double>(4 * ne);   // (nx, ny never change)
  if (!L.sc) L.sc = m.mem.alloc<WallHeatScalars>(1);
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
  wallq_armed = false;
  wallq_plan_upload(std::move(P));
  wallq_opts = o;
  wallq_opts.capacity = cap;
  L.vals = m.wallq_vals;
  L.times = m.wallq_times;
  L.stat = m.wallq_stat;
  L.cap = cap;
  L.statistics = o.statistics ? 1 : 0;
  wallq_reset();
  wallq_armed = true;
}

// The plan of the options over the records the backend holds now.  Throws
// where a value could not be recorded exactly.
WallHeatPlan DeviceSolver::wallq_plan_build(const WallHeatOpts& o) const {
  WallHeatPlan P = build_wall_heat_plan(cs, cs.J, o, l_off);
  for (long c : P.cells)
    if (c < 0 || c >= h.N) throw std::runtime_error("wall heat recorder: a needed cell lies outside the solver's arrays");
  // the lean N-S / mechanism kinds fill a needed cell with the parameters of
  // the recorded step; the fill a download runs takes the next step's, whose
  // is_mu_t differs after the last step before TurbStartIter (the load
  // recorder's refusal, loads_plan_build, and its reasoning)
  if (P.nnodes() > 0 && (lns_ok || lnm_ok) && cs.cfg.ProblemType == SM_NS && !cs.cfg.isTurbulenceReset &&
      cs.cfg.TurbStartIter >= 2 && last_iter + iter < (long)cs.cfg.TurbStartIter)
    throw std::runtime_error("wall heat recorder: wall nodes on the lean N-S / mechanism state cannot be recorded "
                             "exactly before TurbStartIter has passed; arm (or upload) later");
  // a plain lean tile step stores no T, and T = p / R / rho holds only where R
  // does not change over the step; the tile kernel runs its output variant for
  // the probe recorder and the accumulator alone (step_tile.hip)
  if (P.nnodes() > 0 && lean_ok && !lean_sg_ok && make_params(last_iter + iter).chem_model != NO_REACTIONS)
    throw std::runtime_error("wall heat recorder: a reacting gas mixture on the lean inviscid step stores no wall "
                             "temperature between outputs; the recorder cannot be armed on this deck");
  return P;
}

// A built plan into the device arrays (used again where they are large
// enough; the stream is idle: flush_pending / upload synchronised it).
void DeviceSolver::wallq_plan_upload(WallHeatPlan&& P) {
  Impl& m = *impl;
  const long nc = P.ncells(), nn = P.nnodes(), nl = (long)P.list.size();
  const int no = P.nlists() + 1;
  if (nc > m.wallq_cells_cap) {
    m.wallq_cells = m.mem.alloc<long>((size_t)nc);
    m.wallq_scratch = m.mem.alloc<real>(3 * (size_t)nc);
    m.wallq_cells_cap = nc;
  }
  if (nn > m.wallq_nodes_cap) {
    m.wallq_node5 = m.mem.alloc<int>(5 * (size_t)nn);
    m.wallq_nodes_cap = nn;
  }
  if (nl > m.wallq_list_cap) {
    m.wallq_list = m.mem.alloc<int>((size_t)nl);
    m.wallq_list_cap = nl;
  }
  if (!m.wallq_off) m.wallq_off = m.mem.alloc<int>((size_t)no);   // (nx + ny + 1: never changes)
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets, and nothing in flight reads the arrays)
  auto cp = [&](void* d, const void* s, size_t bytes) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, m.stream));
  };
  cp(m.wallq_cells, P.cells.data(), nc * sizeof(long));
  cp(m.wallq_node5, P.node5.data(), 5 * nn * sizeof(int));
  cp(m.wallq_list, P.list.data(), nl * sizeof(int));
  cp(m.wallq_off, P.off.data(), (size_t)no * sizeof(int));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  WallHeatDev& L = m.wallq;
  L.K = P.K;
  L.cells = m.wallq_cells;
  L.node5 = m.wallq_node5;
  L.list = m.wallq_list;
  L.off = m.wallq_off;
  L.scratch = m.wallq_scratch;
  L.ncells = nc;
  L.nx = P.nx;
  L.ny = P.ny;
  wallq_plan = std::move(P);
  wallq_gen++;   // windows captured so far must not replay (mode_signature)
}

// An empty ring and empty statistics whose clock starts at the present value.
void DeviceSolver::wallq_reset() {
  Impl& m = *impl;
  WallHeatScalars s0{};
  s0.s.every = wallq_opts.every;
  s0.s.step_weight = wallq_opts.step_weight ? 1 : 0;
  s0.s.t_off = time_offset;
  HIP_CHECK(hipMemcpyAsync(m.wallq.sc, &s0, sizeof s0, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipMemsetAsync(m.wallq.stat, 0, 4 * (size_t)wallq_plan.nentries() * sizeof(double), m.stream));
  hipLaunchKernelGGL(hf2d_stats_rebase, dim3(1), dim3(64), 0, m.stream, &m.wallq.sc->s, m.sc);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

void DeviceSolver::clear_wall_heat() {
  if (!wallq_armed) return;
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  wallq_reset();
}

WallHeatHistory DeviceSolver::wall_heat_history() {
  if (!wallq_armed) throw std::runtime_error("wall_heat_history: no recorder armed (record_wall_heat)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const WallHeatDev& L = m.wallq;
  const size_t ne = (size_t)wallq_plan.nentries();
  WallHeatScalars ws;
  std::vector<real> vals((size_t)L.cap * ne);
  std::vector<double> tp((size_t)L.cap), stat(4 * ne);
  HIP_CHECK(hipMemcpyAsync(&ws, L.sc, sizeof ws, hipMemcpyDeviceToHost, m.stream));
  if (!vals.empty()) {
    HIP_CHECK(hipMemcpyAsync(vals.data(), L.vals, vals.size() * sizeof(real), hipMemcpyDeviceToHost, m.stream));
    HIP_CHECK(hipMemcpyAsync(tp.data(), L.times, tp.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  }
  HIP_CHECK(hipMemcpyAsync(stat.data(), L.stat, stat.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  // (the probe ring's clock: probe_history)
  return wall_heat_history_from(wallq_plan, wallq_opts, vals.data(), tp.data(), (long)ws.s.samples, stat.data(), ws.s,
                                [&](double t) {
                                  const real part = t - time_offset;
                                  return (double)(cs.global_time + part);
                                });
}

// After the other observers' launches; the same view, and for the lean N-S /
// mechanism state the materialise fill's (as launch_loads).  Nothing here
// allocates, copies or synchronises.
void DeviceSolver::launch_wall_heat(const StepParams& P, int slot, int slot_next) {
  Impl& m = *impl;
  SoA s;
  const int kind = post_step_view(s);
  SoA fin = s, out = s;
  // the dt slot of lns_materialize's fill, which runs after nstep++ (SGL: nstep % 3, else (nstep + 2) % 3)
  int fslot = slot;
  if (lns_state) {
    lns_fill_views(fin, out);
    if (kind == PR_SGL) fslot = slot_next;
  }
  const WallHeatDev& L = m.wallq;
  hipLaunchKernelGGL(hf2d_wallq_tick, dim3(1), dim3(64), 0, m.stream, L.sc, m.sc, L.cap);
  HIP_CHECK(hipGetLastError());
  if (L.ncells > 0) {
    const dim3 g((unsigned)((L.ncells + WALLQ_BLOCK - 1) / WALLQ_BLOCK)), b(WALLQ_BLOCK);
    switch (kind) {
      case PR_SGL: hipLaunchKernelGGL(hf2d_wallq_cells<PR_SGL>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_SGT: hipLaunchKernelGGL(hf2d_wallq_cells<PR_SGT>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_MECH: hipLaunchKernelGGL(hf2d_wallq_cells<PR_MECH>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_LEAN: hipLaunchKernelGGL(hf2d_wallq_cells<PR_LEAN>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      default: hipLaunchKernelGGL(hf2d_wallq_cells<PR_GATHER>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
    }
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(hf2d_wallq_fold, dim3((unsigned)(L.nx + L.ny)), dim3(WALLQ_BLOCK), 0, m.stream, L, m.sc);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Per-step surface recorder (hip/surface_history.hpp)
// ---------------------------------------------------------------------------
void DeviceSolver::record_surface(const SurfaceOpts& o) {
  check_record_surface(o);   // (the options; one strip of several refuses)
  Impl& m = *impl;
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  // (a refused plan throws here and leaves the armed recorder, if any, whole:
  // its options, plan, ring and statistics are replaced only together, below)
  SurfacePlan P = surf_plan_build(o);
  const int cap = (int)std::min<long>(o.capacity, 0x7fffffffL);
  surf_ring_alloc(P, cap);
  SurfaceDev& L = m.surf;
  if (!L.sc) L.sc = m.mem.alloc<WallHeatScalars>(1);
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
  surf_armed = false;
  surf_plan_upload(std::move(P));
  surf_opts = o;
  surf_opts.capacity = cap;
  L.cap = cap;
  L.statistics = o.statistics ? 1 : 0;
  surf_reset();
  surf_armed = true;
}

// The plan of the options over the records the backend holds now.  Throws
// where a value could not be recorded exactly: the wall heat recorder's
// refusals (wallq_plan_build), for the same reasons.
SurfacePlan DeviceSolver::surf_plan_build(const SurfaceOpts& o) const {
  SurfacePlan P = build_surface_plan(cs, cs.J, o, l_off);
  for (long c : P.cells)
    if (c < 0 || c >= h.N) throw std::runtime_error("surface recorder: a needed cell lies outside the solver's arrays");
  if (P.nnodes() > 0 && (lns_ok || lnm_ok) && cs.cfg.ProblemType == SM_NS && !cs.cfg.isTurbulenceReset &&
      cs.cfg.TurbStartIter >= 2 && last_iter + iter < (long)cs.cfg.TurbStartIter)
    throw std::runtime_error("surface recorder: wall nodes on the lean N-S / mechanism state cannot be recorded "
                             "exactly before TurbStartIter has passed; arm (or upload) later");
  if (P.nnodes() > 0 && lean_ok && !lean_sg_ok && make_params(last_iter + iter).chem_model != NO_REACTIONS)
    throw std::runtime_error("surface recorder: a reacting gas mixture on the lean inviscid step stores no wall "
                             "temperature between outputs; the recorder cannot be armed on this deck");
  return P;
}

// Ring and statistics arrays for the plan's node count and `cap` rows (used
// again where they are large enough).
void DeviceSolver::surf_ring_alloc(const SurfacePlan& P, int cap) {
  Impl& m = *impl;
  const size_t ne = (size_t)SURFACE_NVARS * P.nnodes(), nv = (size_t)cap * ne;
  if (nv > m.surf_vals_cap) {
    m.surf_vals = m.mem.alloc<real>(nv);
    m.surf_vals_cap = nv;
  }
  if ((size_t)cap > m.surf_times_cap) {
    m.surf_times = m.mem.alloc<double>((size_t)cap);
    m.surf_times_cap = (size_t)cap;
  }
  if (4 * ne > m.surf_stat_cap) {
    m.surf_stat = m.mem.alloc<double>(4 * ne);
    m.surf_stat_cap = 4 * ne;
  }
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
  m.surf.vals = m.surf_vals;
  m.surf.times = m.surf_times;
  m.surf.stat = m.surf_stat;
}

// A built plan into the device arrays (used again where they are large
// enough; the stream is idle: flush_pending / upload synchronised it).
void DeviceSolver::surf_plan_upload(SurfacePlan&& P) {
  Impl& m = *impl;
  const long nc = P.ncells(), nn = P.nnodes();
  if (nc > m.surf_cells_cap) {
    m.surf_cells = m.mem.alloc<long>((size_t)nc);
    m.surf_mask = m.mem.alloc<uint8_t>((size_t)nc);
    m.surf_scratch = m.mem.alloc<real>((size_t)SURFACE_PLANES * nc);
    m.surf_cells_cap = nc;
  }
  if (nn > m.surf_nodes_cap) {
    m.surf_idx = m.mem.alloc<int>((size_t)SURFACE_IDX * nn);
    m.surf_bits = m.mem.alloc<uint8_t>((size_t)nn);
    m.surf_nodes_cap = nn;
  }
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets, and nothing in flight reads the arrays)
  auto cp = [&](void* d, const void* s, size_t bytes) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, m.stream));
  };
  cp(m.surf_cells, P.cells.data(), nc * sizeof(long));
  cp(m.surf_mask, P.mask.data(), nc * sizeof(uint8_t));
  cp(m.surf_idx, P.idx.data(), (size_t)SURFACE_IDX * nn * sizeof(int));
  cp(m.surf_bits, P.bits.data(), nn * sizeof(uint8_t));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  SurfaceDev& L = m.surf;
  L.K = P.K;
  L.cells = m.surf_cells;
  L.mask = m.surf_mask;
  L.idx = m.surf_idx;
  L.bits = m.surf_bits;
  L.scratch = m.surf_scratch;
  L.ncells = nc;
  L.nnodes = nn;
  surf_plan = std::move(P);
  surf_friction = surf_plan.friction();
  surf_gen++;   // windows captured so far must not replay (mode_signature)
}

// An empty ring and empty statistics whose clock starts at the present value.
void DeviceSolver::surf_reset() {
  Impl& m = *impl;
  WallHeatScalars s0{};
  s0.s.every = surf_opts.every;
  s0.s.step_weight = surf_opts.step_weight ? 1 : 0;
  s0.s.t_off = time_offset;
  HIP_CHECK(hipMemcpyAsync(m.surf.sc, &s0, sizeof s0, hipMemcpyHostToDevice, m.stream));
  const size_t ne = (size_t)SURFACE_NVARS * surf_plan.nnodes();
  if (ne) HIP_CHECK(hipMemsetAsync(m.surf.stat, 0, 4 * ne * sizeof(double), m.stream));
  hipLaunchKernelGGL(hf2d_stats_rebase, dim3(1), dim3(64), 0, m.stream, &m.surf.sc->s, m.sc);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

void DeviceSolver::clear_surface() {
  if (!surf_armed) return;
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  surf_reset();
}

const SurfacePlan& DeviceSolver::surface_plan() const {
  if (!surf_armed) throw std::runtime_error("surface_history: no recorder armed (record_surface)");
  return surf_plan;
}

SurfaceHistory DeviceSolver::surface_history() {
  if (!surf_armed) throw std::runtime_error("surface_history: no recorder armed (record_surface)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const SurfaceDev& L = m.surf;
  const size_t ne = (size_t)SURFACE_NVARS * surf_plan.nnodes();
  WallHeatScalars ws;
  std::vector<real> vals((size_t)L.cap * ne);
  std::vector<double> tp((size_t)L.cap), stat(4 * ne);
  HIP_CHECK(hipMemcpyAsync(&ws, L.sc, sizeof ws, hipMemcpyDeviceToHost, m.stream));
  if (!vals.empty())
    HIP_CHECK(hipMemcpyAsync(vals.data(), L.vals, vals.size() * sizeof(real), hipMemcpyDeviceToHost, m.stream));
  if (!tp.empty())
    HIP_CHECK(hipMemcpyAsync(tp.data(), L.times, tp.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  if (!stat.empty())
    HIP_CHECK(hipMemcpyAsync(stat.data(), L.stat, stat.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  // (the probe ring's clock: probe_history)
  return surface_history_from(surf_plan, surf_opts, vals.data(), tp.data(), (long)ws.s.samples, stat.data(), ws.s,
                              [&](double t) {
                                const real part = t - time_offset;
                                return (double)(cs.global_time + part);
                              });
}

// After the other observers' launches; the same view, and for the lean N-S /
// mechanism state the materialise fill's (as launch_loads).  Nothing here
// allocates, copies or synchronises.
void DeviceSolver::launch_surface(const StepParams& P, int slot, int slot_next) {
  Impl& m = *impl;
  SoA s;
  const int kind = post_step_view(s);
  SoA fin = s, out = s;
  // the dt slot of lns_materialize's fill, which runs after nstep++ (SGL: nstep % 3, else (nstep + 2) % 3)
  int fslot = slot;
  if (lns_state) {
    lns_fill_views(fin, out);
    if (kind == PR_SGL) fslot = slot_next;
  }
  const SurfaceDev& L = m.surf;
  hipLaunchKernelGGL(hf2d_wallq_tick, dim3(1), dim3(64), 0, m.stream, L.sc, m.sc, L.cap);
  HIP_CHECK(hipGetLastError());
  if (L.ncells > 0) {
    const dim3 g((unsigned)((L.ncells + SURF_BLOCK - 1) / SURF_BLOCK)), b(SURF_BLOCK);
    switch (kind) {
      case PR_SGL: hipLaunchKernelGGL(hf2d_surf_cells<PR_SGL>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_SGT: hipLaunchKernelGGL(hf2d_surf_cells<PR_SGT>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_MECH: hipLaunchKernelGGL(hf2d_surf_cells<PR_MECH>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      case PR_LEAN: hipLaunchKernelGGL(hf2d_surf_cells<PR_LEAN>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
      default: hipLaunchKernelGGL(hf2d_surf_cells<PR_GATHER>, g, b, 0, m.stream, P, s, fin, out, L, m.sc, fslot); break;
    }
    HIP_CHECK(hipGetLastError());
  }
  // (at least one workgroup: the sample's time is written for a plan without nodes too)
  const long gn = L.nnodes > 0 ? (L.nnodes + SURF_BLOCK - 1) / SURF_BLOCK : 1;
  hipLaunchKernelGGL(hf2d_surf_nodes, dim3((unsigned)gn), dim3(SURF_BLOCK), 0, m.stream, L, m.sc);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Whole-field time averages (hip/flow_stats.hpp)
// ---------------------------------------------------------------------------
void DeviceSolver::start_averaging(int every, bool second_moments, bool step_weight, bool favre,
                                   const std::vector<int>& species) {
  check_averaging(every, species, h.nsp);
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const size_t N = (size_t)h.N, planes = stats_plane_count(second_moments, favre, (int)species.size());
  FlowStats f = m.stats;
  if (planes > m.stats_planes) {   // (arming again with as many planes or fewer reuses them)
    f.m = m.mem.alloc<double>(planes * N);
    m.stats_planes = planes;
  }
  if (!f.sc) f.sc = m.mem.alloc<StatsScalars>(1);
  f.M = second_moments ? f.m + STATS_VARS * N : nullptr;
  f.C = second_moments ? f.m + 2 * STATS_VARS * N : nullptr;
  f.c0 = (long)l_off * h.ny;
  f.c1 = f.c0 + (long)(gi1 - gi0) * h.ny;
  StatsExt x{};
  x.ns = (int)species.size();
  std::copy(species.begin(), species.end(), x.sp);
  stats_ext_planes(x, f.m, N, second_moments, favre);
  HIP_CHECK(hipDeviceSynchronize());   // (the allocator's memsets)
  StatsScalars s0{};
  s0.every = every;
  s0.step_weight = step_weight ? 1 : 0;
  s0.t_off = time_offset;
  HIP_CHECK(hipMemcpyAsync(f.sc, &s0, sizeof s0, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipMemsetAsync(f.m, 0, planes * N * sizeof(double), m.stream));
  hipLaunchKernelGGL(hf2d_stats_rebase, dim3(1), dim3(64), 0, m.stream, f.sc, m.sc);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(m.stream));
  m.stats = f;
  m.stats_x = x;
  m.stats_used = planes;
  stats_second = second_moments;
  stats_favre = favre;
  stats_species = species;
  stats_on = stats_armed = true;
  stats_gen++;   // windows captured so far must not replay (mode_signature)
}

void DeviceSolver::reset_averaging() {
  if (!stats_on) return;
  flush_pending();
  Impl& m = *impl;
  HIP_CHECK(hipMemsetAsync(m.stats.m, 0, m.stats_used * (size_t)h.N * sizeof(double), m.stream));
  hipLaunchKernelGGL(hf2d_stats_rebase, dim3(1), dim3(64), 0, m.stream, m.stats.sc, m.sc);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

void DeviceSolver::stop_averaging() {
  if (!stats_on) return;
  flush_pending();
  stats_on = false;
  stats_gen++;   // the cached windows hold the accumulate nodes
}

FlowAverages DeviceSolver::averages() {
  if (!stats_armed) throw std::runtime_error("averages: no accumulator armed (start_averaging)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const FlowStats& f = m.stats;
  const StatsExt& x = m.stats_x;
  FlowAverages A;
  A.gi0 = gi0;
  A.gi1 = gi1;
  A.ny = h.ny;
  A.second_moments = stats_second;
  A.favre = stats_favre;
  A.species = stats_species;
  const size_t n = (size_t)(f.c1 - f.c0), N = (size_t)h.N;
  StatsScalars sc;
  HIP_CHECK(hipMemcpyAsync(&sc, f.sc, sizeof sc, hipMemcpyDeviceToHost, m.stream));
  auto planes = [&](const double* src, int np, std::vector<double>& dst) {
    dst.resize((size_t)np * n);
    for (int k = 0; k < np; k++)
      HIP_CHECK(hipMemcpyAsync(dst.data() + k * n, src + k * N + f.c0, n * sizeof(double), hipMemcpyDeviceToHost,
                               m.stream));
  };
  const int ns = x.ns, nf = STATS_FAVRE_BASE + ns;
  planes(f.m, STATS_VARS, A.mean);
  planes(x.mY, ns, A.species_mean);
  if (stats_favre) {
    planes(x.G, 1, A.favre_weight);
    planes(x.f, nf, A.favre_mean);
  }
  if (stats_second) {
    planes(f.M, STATS_VARS, A.var);
    planes(f.C, 1, A.cov_uv);
    planes(x.MY, ns, A.species_var);
    if (stats_favre) {
      planes(x.F, nf, A.favre_var);
      planes(x.CF, 1, A.favre_cov_uv);
    }
  }
  HIP_CHECK(hipStreamSynchronize(m.stream));
  A.time = sc.W;
  A.samples = (long)sc.samples;
  if (stats_second) A.finish(sc.W);
  return A;
}

// After the recorder's launch: the tick decides on the device whether the
// step is a sample and forms its weight; the cell pass reads the same view
// the recorder reads.  Nothing here allocates, copies or synchronises.
template <int KIND>
static void launch_stats_kind(hipStream_t st, unsigned nblk, bool second, const StepParams& P, const SoA& s,
                              const FlowStats& f) {
  if (second)
    hipLaunchKernelGGL((hf2d_stats_accum<KIND, true>), dim3(nblk), dim3(STATS_BLOCK), 0, st, P, s, f);
  else
    hipLaunchKernelGGL((hf2d_stats_accum<KIND, false>), dim3(nblk), dim3(STATS_BLOCK), 0, st, P, s, f);
}

// the same pass with Favre averages or species statistics armed
template <int KIND>
static void launch_stats_x_kind(hipStream_t st, unsigned nblk, bool second, bool favre, const StepParams& P,
                                const SoA& s, const FlowStats& f, const StatsExt& x) {
  const dim3 g(nblk), b(STATS_BLOCK);
  if (second && favre)
    hipLaunchKernelGGL((hf2d_stats_accum_x<KIND, true, true>), g, b, 0, st, P, s, f, x);
  else if (second)
    hipLaunchKernelGGL((hf2d_stats_accum_x<KIND, true, false>), g, b, 0, st, P, s, f, x);
  else if (favre)
    hipLaunchKernelGGL((hf2d_stats_accum_x<KIND, false, true>), g, b, 0, st, P, s, f, x);
  else
    hipLaunchKernelGGL((hf2d_stats_accum_x<KIND, false, false>), g, b, 0, st, P, s, f, x);
}

void DeviceSolver::launch_stats(const StepParams& P) {
  Impl& m = *impl;
  SoA s;
  const int kind = post_step_view(s);
  const FlowStats& f = m.stats;
  hipLaunchKernelGGL(hf2d_stats_tick, dim3(1), dim3(64), 0, m.stream, f.sc, m.sc);
  HIP_CHECK(hipGetLastError());
  const unsigned nblk = (unsigned)((f.c1 - f.c0 + STATS_BLOCK - 1) / STATS_BLOCK);
  if (stats_favre || m.stats_x.ns > 0) {
    const StatsExt& x = m.stats_x;
    // (a listed species is a plane of the view's block: check_averaging)
    if (x.ns > 0 && (!s.Ys || s.nsp != h.nsp)) throw std::runtime_error("flow statistics: the step's view holds no species block");
    switch (kind) {
      case PR_SGL: launch_stats_x_kind<PR_SGL>(m.stream, nblk, stats_second, stats_favre, P, s, f, x); break;
      case PR_SGT: launch_stats_x_kind<PR_SGT>(m.stream, nblk, stats_second, stats_favre, P, s, f, x); break;
      case PR_MECH: launch_stats_x_kind<PR_MECH>(m.stream, nblk, stats_second, stats_favre, P, s, f, x); break;
      case PR_LEAN: launch_stats_x_kind<PR_LEAN>(m.stream, nblk, stats_second, stats_favre, P, s, f, x); break;
      default: launch_stats_x_kind<PR_GATHER>(m.stream, nblk, stats_second, stats_favre, P, s, f, x); break;
    }
    HIP_CHECK(hipGetLastError());
    return;
  }
  switch (kind) {
    case PR_SGL: launch_stats_kind<PR_SGL>(m.stream, nblk, stats_second, P, s, f); break;
    case PR_SGT: launch_stats_kind<PR_SGT>(m.stream, nblk, stats_second, P, s, f); break;
    case PR_MECH: launch_stats_kind<PR_MECH>(m.stream, nblk, stats_second, P, s, f); break;
    case PR_LEAN: launch_stats_kind<PR_LEAN>(m.stream, nblk, stats_second, P, s, f); break;
    default: launch_stats_kind<PR_GATHER>(m.stream, nblk, stats_second, P, s, f); break;
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace hf2d
