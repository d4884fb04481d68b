// Observers of the run: monitor points, the per-step probe recorder
// (probe_history.hpp), the per-step load recorder (load_history.hpp), the
// per-step wall heat recorder (wall_heat.hpp), the per-step surface recorder
// (surface_history.hpp), the per-step frame recorder (frame_history.hpp) and the
// time-averaged flow statistics (flow_stats.hpp).

#include "device_impl.hpp"
#include "flow_stats.hpp"
#include "load_history.hpp"
#include "wall_heat.hpp"
#include "surface_history.hpp"
#include "frame_history.hpp"

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
  HIP_CHECK(hipDeviceSynchronize());   // (the steps flush_pending launched: nothing in flight reads the arrays)
  auto& a = m.ring_mem;
  r.idx = m.plan_array(a.idx, probe_rec_idx);
  r.rows = m.grown(a.rows, (size_t)r.cap * n * PROBE_VARS);
  r.times = m.grown(a.times, (size_t)r.cap);
  r.count = m.grown(a.count, 1);
  HIP_CHECK(hipMemsetAsync(r.count, 0, sizeof(unsigned long long), m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  m.ring = r;
  probe_cap = r.cap;
  observers_gen++;
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
  ring_oldest_first(rows.data(), row, tp.data(), H.total, (long)r.cap, [&](double t) { return host_time(t); },
                    H.values, H.times);
  H.owned.resize(r.n);
  for (int q = 0; q < r.n; q++) H.owned[q] = probe_rec_idx[q] >= 0 ? 1 : 0;
  return H;
}

// The device accumulates time since the cycle start (on_cycle_roll moved the
// stored times of earlier cycles with it); the host's time is
// global_time + (time_part - time_offset) (sync_scalars, summary).
double DeviceSolver::host_time(double t_dev) const {
  const real part = t_dev - time_offset;
  return (double)(cs.global_time + part);
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

// ... and with it, for the lean N-S / mechanism state, the views and the dt
// slot of lns_materialize's fill, which runs after nstep++ (SGL: nstep % 3,
// else (nstep + 2) % 3).  Once per step, for every observer that is armed.
PostStep DeviceSolver::post_step(int slot, int slot_next) const {
  PostStep v;
  v.kind = post_step_view(v.s);
  v.fin = v.out = v.s;
  v.fslot = slot;
  if (lns_state) {
    lns_fill_views(v.fin, v.out);
    if (v.kind == PR_SGL) v.fslot = slot_next;
  }
  return v;
}

void DeviceSolver::launch_probe_record(const StepParams& P, const PostStep& v) {
  Impl& m = *impl;
  with_kind(v.kind, [&](auto K) {
    hipLaunchKernelGGL(hf2d_probe_record<decltype(K)::value>, dim3(1), dim3(PROBE_MAX), 0, m.stream, P, v.s, m.ring, m.sc);
  });
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
  LoadsDev& L = m.loads;
  auto& a = m.loads_mem;
  HIP_CHECK(hipDeviceSynchronize());   // (the steps flush_pending launched: nothing in flight reads the arrays)
  loads_cap = 0;
  L.vals = m.grown(a.vals, (size_t)cap * P.nlists());
  L.times = m.grown(a.times, (size_t)cap);
  L.count = m.grown(a.count, 1);
  L.cap = cap;
  loads_plan_upload(std::move(P));
  loads_boxes = boxes;
  loads_cuts = cuts;
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
  // (the box terms are the wall nodes', and they read no wall temperature)
  if (P.off[(size_t)LOAD_PARTS * P.nboxes] > 0) refuse_wall_nodes("load recorder", "wall terms", false);
  return P;
}

// The two rules that refuse a plan with wall nodes, in the words of the
// recorder `who`, which calls them `nodes`; wall_T: it reads their temperature.
void DeviceSolver::refuse_wall_nodes(const std::string& who, const char* nodes, bool wall_T) const {
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
  if ((lns_ok || lnm_ok) && cs.cfg.ProblemType == SM_NS && !cs.cfg.isTurbulenceReset && cs.cfg.TurbStartIter >= 2 &&
      last_iter + iter < (long)cs.cfg.TurbStartIter)
    throw std::runtime_error(who + ": " + nodes + " on the lean N-S / mechanism state cannot be recorded exactly before "
                                                  "TurbStartIter has passed; arm (or upload) later");
  // a plain lean tile step stores no T, and T = p / R / rho holds only where R
  // does not change over the step; the tile kernel runs its output variant for
  // the probe recorder, the accumulator and the frame recorder alone (step_tile.hip)
  if (wall_T && lean_ok && !lean_sg_ok && make_params(last_iter + iter).chem_model != NO_REACTIONS)
    throw std::runtime_error(who + ": a reacting gas mixture on the lean inviscid step stores no wall temperature between "
                                   "outputs; the recorder cannot be armed on this deck");
}

// A built plan into the device arrays (used again where they are large
// enough; the stream is idle: flush_pending / upload synchronised it).
void DeviceSolver::loads_plan_upload(LoadPlan&& P) {
  Impl& m = *impl;
  auto& a = m.loads_mem;
  LoadsDev& L = m.loads;
  L.nterms = P.nterms();
  L.nlists = P.nlists();
  L.scratch = m.grown(a.scratch, (size_t)L.nterms);
  L.cell = m.plan_array(a.cell, P.cell);
  L.cell2 = m.plan_array(a.cell2, P.cell2);
  L.coef = m.plan_array(a.coef, P.coef);
  L.kind = m.plan_array(a.kind, P.kind);
  L.off = m.plan_array(a.off, P.off);
  HIP_CHECK(hipStreamSynchronize(m.stream));
  loads_plan = std::move(P);
  loads_friction = loads_plan.friction();
  observers_gen++;
}

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
  return load_history_from_ring(loads_plan, vals.data(), tp.data(), (long)total, (long)L.cap,
                                [&](double t) { return host_time(t); });
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

// (no term kernel of the PR_LEAN kind: a term reads no T, and the lean inviscid
// arrays store everything else per cell, load_history.hpp)
void DeviceSolver::launch_loads(const StepParams& P, const PostStep& v) {
  Impl& m = *impl;
  const LoadsDev& L = m.loads;
  if (L.nterms > 0) {
    const dim3 g((unsigned)((L.nterms + LOADS_BLOCK - 1) / LOADS_BLOCK)), b(LOADS_BLOCK);
    with_kind<false>(v.kind, [&](auto K) {
      hipLaunchKernelGGL(hf2d_loads_terms<decltype(K)::value>, g, b, 0, m.stream, P, v.s, v.fin, v.out, L, m.sc, v.fslot);
    });
    HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(hf2d_loads_fold, dim3(1), dim3(LOADS_FOLD_WAVES * WAVE), 0, m.stream, L, m.sc);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// The sampled ring of the wall heat and the surface recorder (SampleRing)
// ---------------------------------------------------------------------------
// An empty ring and empty statistics whose clock starts at the present value.
void DeviceSolver::Impl::ring_reset(const SampleRing& r, size_t ne, int every, bool step_weight, double t_off) {
  WallHeatScalars s0{};
  s0.s.every = every;
  s0.s.step_weight = step_weight ? 1 : 0;
  s0.s.t_off = t_off;
  HIP_CHECK(hipMemcpyAsync(r.sc, &s0, sizeof s0, hipMemcpyHostToDevice, stream));
  if (ne) HIP_CHECK(hipMemsetAsync(r.stat, 0, 4 * ne * sizeof(double), stream));
  hipLaunchKernelGGL(hf2d_stats_rebase, dim3(1), dim3(64), 0, stream, &r.sc->s, sc);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(stream));
}

SampledRing DeviceSolver::Impl::ring_read(const SampleRing& r, size_t ne) {
  SampledRing R;
  WallHeatScalars ws;
  R.vals.resize((size_t)r.cap * ne);
  R.times.resize((size_t)r.cap);
  R.stat.resize(4 * ne);
  auto get = [&](void* d, const void* s, size_t bytes) {
    if (bytes) HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, stream));
  };
  get(&ws, r.sc, sizeof ws);
  get(R.vals.data(), r.vals, R.vals.size() * sizeof(real));
  get(R.times.data(), r.times, R.times.size() * sizeof(double));
  get(R.stat.data(), r.stat, R.stat.size() * sizeof(double));
  HIP_CHECK(hipStreamSynchronize(stream));
  R.sc = ws.s;
  R.total = (long)ws.s.samples;
  return R;
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
  HIP_CHECK(hipDeviceSynchronize());   // (the steps flush_pending launched: nothing in flight reads the arrays)
  wallq_armed = false;
  SampleRing& r = m.wallq.ring;
  m.ring_alloc(m.wallq_mem.ring, r, (size_t)P.nentries(), (int)std::min<long>(o.capacity, 0x7fffffffL));
  r.statistics = o.statistics ? 1 : 0;
  wallq_plan_upload(std::move(P));
  wallq_opts = o;
  wallq_opts.capacity = r.cap;
  m.ring_reset(r, (size_t)wallq_plan.nentries(), o.every, o.step_weight, time_offset);
  wallq_armed = true;
}

// The plan of the options over the records the backend holds now.  Throws
// where a value could not be recorded exactly.
WallHeatPlan DeviceSolver::wallq_plan_build(const WallHeatOpts& o) const {
  WallHeatPlan P = build_wall_heat_plan(cs, cs.J, o, l_off);
  for (long c : P.cells)
    if (c < 0 || c >= h.N) throw std::runtime_error("wall heat recorder: a needed cell lies outside the solver's arrays");
  if (P.nnodes() > 0) refuse_wall_nodes("wall heat recorder", "wall nodes", true);
  return P;
}

// A built plan into the device arrays (used again where they are large
// enough; the stream is idle: flush_pending / upload synchronised it).
void DeviceSolver::wallq_plan_upload(WallHeatPlan&& P) {
  Impl& m = *impl;
  auto& a = m.wallq_mem;
  WallHeatDev& L = m.wallq;
  L.K = P.K;
  L.ncells = P.ncells();
  L.nx = P.nx;
  L.ny = P.ny;
  L.scratch = m.grown(a.scratch, 3 * (size_t)L.ncells);
  L.cells = m.plan_array(a.cells, P.cells);
  L.node5 = m.plan_array(a.node5, P.node5);
  L.list = m.plan_array(a.list, P.list);
  L.off = m.plan_array(a.off, P.off);
  HIP_CHECK(hipStreamSynchronize(m.stream));
  wallq_plan = std::move(P);
  observers_gen++;
}

void DeviceSolver::clear_wall_heat() {
  if (!wallq_armed) return;
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  impl->ring_reset(impl->wallq.ring, (size_t)wallq_plan.nentries(), wallq_opts.every, wallq_opts.step_weight, time_offset);
}

WallHeatHistory DeviceSolver::wall_heat_history() {
  if (!wallq_armed) throw std::runtime_error("wall_heat_history: no recorder armed (record_wall_heat)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  return wall_heat_history_from(wallq_plan, wallq_opts, impl->ring_read(impl->wallq.ring, (size_t)wallq_plan.nentries()),
                                [&](double t) { return host_time(t); });
}

void DeviceSolver::launch_wall_heat(const StepParams& P, const PostStep& v) {
  Impl& m = *impl;
  const WallHeatDev& L = m.wallq;
  hipLaunchKernelGGL(hf2d_wallq_tick, dim3(1), dim3(64), 0, m.stream, L.ring.sc, m.sc, L.ring.cap);
  HIP_CHECK(hipGetLastError());
  if (L.ncells > 0) {
    const dim3 g((unsigned)((L.ncells + WALLQ_BLOCK - 1) / WALLQ_BLOCK)), b(WALLQ_BLOCK);
    with_kind(v.kind, [&](auto K) {
      hipLaunchKernelGGL(hf2d_wallq_cells<decltype(K)::value>, g, b, 0, m.stream, P, v.s, v.fin, v.out, L, m.sc, v.fslot);
    });
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
  HIP_CHECK(hipDeviceSynchronize());   // (the steps flush_pending launched: nothing in flight reads the arrays)
  surf_armed = false;
  SampleRing& r = m.surf.ring;
  m.ring_alloc(m.surf_mem.ring, r, P.nentries(), (int)std::min<long>(o.capacity, 0x7fffffffL));
  r.statistics = o.statistics ? 1 : 0;
  surf_plan_upload(std::move(P));
  surf_opts = o;
  surf_opts.capacity = r.cap;
  m.ring_reset(r, surf_plan.nentries(), o.every, o.step_weight, time_offset);
  surf_armed = true;
}

// The plan of the options over the records the backend holds now.  Throws
// where a value could not be recorded exactly.
SurfacePlan DeviceSolver::surf_plan_build(const SurfaceOpts& o) const {
  SurfacePlan P = build_surface_plan(cs, cs.J, o, l_off);
  for (long c : P.cells)
    if (c < 0 || c >= h.N) throw std::runtime_error("surface recorder: a needed cell lies outside the solver's arrays");
  if (P.nnodes() > 0) refuse_wall_nodes("surface recorder", "wall nodes", true);
  return P;
}

// A built plan into the device arrays (used again where they are large
// enough; the stream is idle: flush_pending / upload synchronised it).
void DeviceSolver::surf_plan_upload(SurfacePlan&& P) {
  Impl& m = *impl;
  auto& a = m.surf_mem;
  SurfaceDev& L = m.surf;
  L.K = P.K;
  L.ncells = P.ncells();
  L.nnodes = P.nnodes();
  L.scratch = m.grown(a.scratch, (size_t)SURFACE_PLANES * L.ncells);
  L.cells = m.plan_array(a.cells, P.cells);
  L.mask = m.plan_array(a.mask, P.mask);
  L.idx = m.plan_array(a.idx, P.idx);
  L.bits = m.plan_array(a.bits, P.bits);
  HIP_CHECK(hipStreamSynchronize(m.stream));
  surf_plan = std::move(P);
  surf_friction = surf_plan.friction();
  observers_gen++;
}

void DeviceSolver::clear_surface() {
  if (!surf_armed) return;
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  impl->ring_reset(impl->surf.ring, surf_plan.nentries(), surf_opts.every, surf_opts.step_weight, time_offset);
}

const SurfacePlan& DeviceSolver::surface_plan() const {
  if (!surf_armed) throw std::runtime_error("surface_history: no recorder armed (record_surface)");
  return surf_plan;
}

SurfaceHistory DeviceSolver::surface_history() {
  if (!surf_armed) throw std::runtime_error("surface_history: no recorder armed (record_surface)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  return surface_history_from(surf_plan, surf_opts, impl->ring_read(impl->surf.ring, surf_plan.nentries()),
                              [&](double t) { return host_time(t); });
}

void DeviceSolver::launch_surface(const StepParams& P, const PostStep& v) {
  Impl& m = *impl;
  const SurfaceDev& L = m.surf;
  hipLaunchKernelGGL(hf2d_wallq_tick, dim3(1), dim3(64), 0, m.stream, L.ring.sc, m.sc, L.ring.cap);
  HIP_CHECK(hipGetLastError());
  if (L.ncells > 0) {
    const dim3 g((unsigned)((L.ncells + SURF_BLOCK - 1) / SURF_BLOCK)), b(SURF_BLOCK);
    with_kind(v.kind, [&](auto K) {
      hipLaunchKernelGGL(hf2d_surf_cells<decltype(K)::value>, g, b, 0, m.stream, P, v.s, v.fin, v.out, L, m.sc, v.fslot);
    });
    HIP_CHECK(hipGetLastError());
  }
  // (at least one workgroup: the sample's time is written for a plan without nodes too)
  const long gn = L.nnodes > 0 ? (L.nnodes + SURF_BLOCK - 1) / SURF_BLOCK : 1;
  hipLaunchKernelGGL(hf2d_surf_nodes, dim3((unsigned)gn), dim3(SURF_BLOCK), 0, m.stream, L, m.sc);
  HIP_CHECK(hipGetLastError());
}

// ---------------------------------------------------------------------------
// Per-step frame recorder (hip/frame_history.hpp)
// ---------------------------------------------------------------------------
// No plan: the kernels read CT live, so upload() rebuilds nothing.
void DeviceSolver::record_frames(const FrameOpts& o) {
  // (a refused call throws here and leaves the armed recorder, if any, whole)
  const FrameGeom G = check_record_frames(o, l_off);
  Impl& m = *impl;
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  HIP_CHECK(hipDeviceSynchronize());   // (the steps flush_pending launched: nothing in flight reads the arrays)
  frames_armed = false;
  FrameDev& L = m.frames;
  auto& a = m.frames_mem;
  SampleRing& r = L.ring;
  const int cap = (int)std::min<long>(o.capacity, 0x7fffffffL);
  r.vals = m.grown(a.ring.vals, (size_t)cap * G.nvars * G.ncells());
  r.times = m.grown(a.ring.times, (size_t)cap);
  r.sc = m.grown(a.ring.sc, 1);
  r.stat = nullptr;
  r.cap = cap;
  r.statistics = 0;
  L.scratch = m.grown(a.scratch, (size_t)FRAME_ROW * G.nbox());
  L.G = G;
  frames_opts = o;
  frames_opts.capacity = cap;
  m.ring_reset(r, 0, o.every, true, time_offset);
  frames_armed = true;
  observers_gen++;
}

void DeviceSolver::clear_frames() {
  if (!frames_armed) return;
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  impl->ring_reset(impl->frames.ring, 0, frames_opts.every, true, time_offset);
  observers_gen++;
}

FrameHistory DeviceSolver::frame_history() {
  if (!frames_armed) throw std::runtime_error("frame_history: no recorder armed (record_frames)");
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  const FrameDev& L = m.frames;
  const FrameGeom& G = L.G;
  const size_t ne = (size_t)G.nvars * G.ncells();
  WallHeatScalars ws;
  std::vector<real> vals((size_t)L.ring.cap * ne);
  std::vector<double> tp((size_t)L.ring.cap);
  HIP_CHECK(hipMemcpyAsync(&ws, L.ring.sc, sizeof ws, hipMemcpyDeviceToHost, m.stream));
  if (!vals.empty())
    HIP_CHECK(hipMemcpyAsync(vals.data(), L.ring.vals, vals.size() * sizeof(real), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipMemcpyAsync(tp.data(), L.ring.times, tp.size() * sizeof(double), hipMemcpyDeviceToHost, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
  FrameHistory H;
  H.G = G;
  H.total = (long)ws.s.samples;
  ring_oldest_first(vals.data(), ne, tp.data(), H.total, (long)L.ring.cap, [&](double t) { return host_time(t); },
                    H.vals, H.times);
  H.gas.resize((size_t)G.ncells());
  for (int a = 0; a < G.ni; a++)
    for (int b = 0; b < G.nj; b++)
      H.gas[(size_t)a * G.nj + b] = frame_gas(h.CT[(long)(G.i0 + a * G.si + G.ioff) * h.ny + G.j0 + b * G.sj]) ? 1 : 0;
  return H;
}

void DeviceSolver::launch_frames(const StepParams& P, const PostStep& v) {
  Impl& m = *impl;
  const FrameDev& L = m.frames;
  hipLaunchKernelGGL(hf2d_wallq_tick, dim3(1), dim3(64), 0, m.stream, L.ring.sc, m.sc, L.ring.cap);
  HIP_CHECK(hipGetLastError());
  if (L.G.nbox() > 0) {
    const dim3 g((unsigned)((L.G.nbox() + FRAME_BLOCK - 1) / FRAME_BLOCK)), b(FRAME_BLOCK);
    with_kind(v.kind, [&](auto K) {
      hipLaunchKernelGGL(hf2d_frame_rows<decltype(K)::value>, g, b, 0, m.stream, P, v.s, L);
    });
    HIP_CHECK(hipGetLastError());
  }
  // (at least one workgroup: the sample's time is written for a strip without output columns too)
  const long gn = L.G.ncells() > 0 ? (L.G.ncells() + FRAME_BLOCK - 1) / FRAME_BLOCK : 1;
  hipLaunchKernelGGL(hf2d_frame_store, dim3((unsigned)gn), dim3(FRAME_BLOCK), 0, m.stream, L, v.s.CT, v.s.N, m.sc);
  HIP_CHECK(hipGetLastError());
}

// upload() replaced the records under the armed recorders: the same targets
// and options over the new flags.  The load ring keeps its shape (as many
// lists as before) and so does the wall heat ring (nx, ny never change);
// another node count restarts the surface recorder's ring and statistics.
void DeviceSolver::plans_rebuild() {
  Impl& m = *impl;
  if (loads_cap) loads_plan_upload(loads_plan_build(loads_boxes, loads_cuts));
  if (wallq_armed) wallq_plan_upload(wallq_plan_build(wallq_opts));
  if (!surf_armed) return;
  const size_t ne = surf_plan.nentries();
  surf_plan_upload(surf_plan_build(surf_opts));
  if (surf_plan.nentries() == ne) return;
  m.ring_alloc(m.surf_mem.ring, m.surf.ring, surf_plan.nentries(), m.surf.ring.cap);
  m.ring_reset(m.surf.ring, surf_plan.nentries(), surf_opts.every, surf_opts.step_weight, time_offset);
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
  observers_gen++;
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
  observers_gen++;   // the cached windows hold the accumulate nodes
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

void DeviceSolver::launch_stats(const StepParams& P, const PostStep& v) {
  Impl& m = *impl;
  const SoA& s = v.s;
  const FlowStats& f = m.stats;
  hipLaunchKernelGGL(hf2d_stats_tick, dim3(1), dim3(64), 0, m.stream, f.sc, m.sc);
  HIP_CHECK(hipGetLastError());
  const unsigned nblk = (unsigned)((f.c1 - f.c0 + STATS_BLOCK - 1) / STATS_BLOCK);
  if (stats_favre || m.stats_x.ns > 0) {
    const StatsExt& x = m.stats_x;
    // (a listed species is a plane of the view's block: check_averaging)
    if (x.ns > 0 && (!s.Ys || s.nsp != h.nsp)) throw std::runtime_error("flow statistics: the step's view holds no species block");
    with_kind(v.kind, [&](auto K) {
      launch_stats_x_kind<decltype(K)::value>(m.stream, nblk, stats_second, stats_favre, P, s, f, x);
    });
  } else {
    with_kind(v.kind, [&](auto K) { launch_stats_kind<decltype(K)::value>(m.stream, nblk, stats_second, P, s, f); });
  }
  HIP_CHECK(hipGetLastError());
}

}  // namespace hf2d
