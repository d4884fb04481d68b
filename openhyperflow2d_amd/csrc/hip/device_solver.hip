// GPU backend for MI355X (gfx950): device-resident SoA state, one HIP
// kernel per DEEPS phase, RCCL halo exchange / reductions for strip-
// decomposed multi-GPU runs.
//
// One translation unit per group of kernel families; each holds its kernels, their
// tables and the DeviceSolver members that launch them, and every __global__
// is compiled in exactly one of them:
//   device_solver.hip   this file: construction, upload / download, the step
//                       dispatcher and its graphs, scalars read-back
//                       (hf2d_scalars_out), residual reduction, autotune
//   step_tile.hip       inviscid lean steps: lean_tile.hpp (hf2d_lean_tile*),
//                       flat lean Euler, lean materialize
//   step_ns.hip         the N-S and split steps, one unit because their kernels
//                       share the fill (see the file): split predict / fill,
//                       fused Euler, generic kinetics, wall heat, y+; lean N-S
//                       tile step (hf2d_lns_step*; lean_ns.hpp: arrays, LDS
//                       layout, per-cell functions); lean mechanism tile step
//                       (hf2d_lnm_*; lean_mech.hpp likewise)
//   transport.hip       halo_kernels.hpp: halo pack / unpack, dt fold, xGMI
//                       mailbox kernels (hf2d_p2p_*); RCCL and in-process transports
//   observe.hip         monitors and the six per-step observers: probe_history.hpp,
//                       load_history.hpp, wall_heat.hpp, surface_history.hpp,
//                       frame_history.hpp (recorders),
//                       flow_stats.hpp (time-averaged flow statistics)
//   device_knobs.hpp    the tuning knobs, one row each: members, environment reads,
//                       Python attributes and mode_signature() are expanded from it
//   device_impl.hpp     DeviceSolver::Impl, DevBuf, HIP_CHECK: what the units share
//   solver_args.hpp     plain argument blocks of the lean N-S / mechanism steps
//                       and the recorder (types only)
//   dev_common.hpp      device-side scalars, dt slots and the fused-exchange
//                       pieces several families use (no __global__)
// dt never leaves the device inside the inner loop: hf2d_fill folds the
// local CFL limit into a device slot with an integer atomicMin on the IEEE
// bits (valid for positive doubles, order independent => deterministic) and
// the next step's kernels read it from there.

#include "device_impl.hpp"

namespace hf2d {

__global__ __launch_bounds__(BLOCK) void hf2d_reduce_residual(const ResidualPack* partials, long n,
                                                               ResidualPack* outp) {
  __shared__ ResidualPack sh[32];
  ResidualPack acc;
  residual_reset(acc);
  for (int k = 0; k < NEQ; k++) acc.eq[k].i = acc.eq[k].j = -1;
  for (long t = threadIdx.x; t < n; t += BLOCK) residual_merge_lex(acc, partials[t]);
  for (int off = 1; off < WAVE; off <<= 1) shfl_merge(acc, off);
  const int w = threadIdx.x / WAVE;
  if ((threadIdx.x & (WAVE - 1)) == 0) sh[w] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    ResidualPack a = sh[0];
    for (int q = 1; q < BLOCK / WAVE; q++) residual_merge_lex(a, sh[q]);
    *outp = a;
  }
}

// The scalars the host reads (the words before the dt shards, and the shards
// of the dt slot it reads) into pinned host memory with plain vector stores,
// queued behind the step's kernels: the host then waits for the stream only,
// instead of for the stream and a device-to-host copy of the whole block behind
// it (one copy-engine round trip per sync_scalars, i.e. per run_steps call).
__global__ __launch_bounds__(WAVE) void hf2d_scalars_out(const DevScalars* sc, DevScalars* host, int slot) {
  constexpr int NH = (int)(offsetof(DevScalars, dt_sh) / 8);
  static_assert(offsetof(DevScalars, dt_sh) % 8 == 0 && NH <= WAVE, "DevScalars header is copied in 8-byte words");
  const unsigned long long* src = reinterpret_cast<const unsigned long long*>(sc);
  unsigned long long* dst = reinterpret_cast<unsigned long long*>(host);
  const int t = threadIdx.x;
  if (t < NH) dst[t] = src[t];
  if (t < DT_SHARDS) host->dt_sh[slot][t][0] = sc->dt_sh[slot][t][0];
}

static int g_device_count_cache = -1;

bool gpu_available() {
  if (g_device_count_cache < 0) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    g_device_count_cache = n;
  }
  return g_device_count_cache > 0;
}

DeviceSolver::DeviceSolver(Case& c, int device, int gi0_, int gi1_) : SolverBase(c), impl(new Impl) {
  if (!gpu_available()) throw std::runtime_error("no HIP device available");
  dev = device;
  HIP_CHECK(hipSetDevice(dev));
  HIP_CHECK(hipStreamCreateWithFlags(&impl->stream, hipStreamNonBlocking));
  {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    cu_count = prop.multiProcessorCount;
  }
  read_env();
  gi0 = gi0_;
  gi1 = gi1_ < 0 ? c.J.nx : gi1_;
  // ghost columns: N-S strips keep two (the lean N-S / mechanism tiles
  // evaluate the fill of the first ghost column, which reads the second);
  // the split kernels read one, the inviscid ones one
  const int G = c.cfg.ProblemType == SM_NS ? 2 : 1;
  const int lh = gi0 > 0 ? G : 0, rh = gi1 < c.J.nx ? G : 0;
  l_off = lh;
  h.allocate((gi1 - gi0) + lh + rh, c.J.ny);
  const long N = h.N;
  Impl& m = *impl;
  for (int b = 0; b < 2; b++) {
    m.S[b] = m.mem.alloc<real>(NEQ * N);
    m.A[b] = m.mem.alloc<real>(NEQ * N);
    m.B[b] = m.mem.alloc<real>(NEQ * N);
    m.dSdx[b] = m.mem.alloc<real>(NEQ * N);
    m.dSdy[b] = m.mem.alloc<real>(NEQ * N);
    m.U[b] = m.mem.alloc<real>(N);
    m.V[b] = m.mem.alloc<real>(N);
    m.Tg[b] = m.mem.alloc<real>(N);
    m.Spre[b] = m.mem.alloc<real>(NCOMP * N);
    m.P2[b] = m.mem.alloc<real>(N);
  }
  m.lb = m.mem.alloc<uint8_t>(N);
  m.gf = m.mem.alloc<uint8_t>(N);
  m.F = m.mem.alloc<real>(NEQ * N);
  m.Src = m.mem.alloc<real>(NEQ * N);
  m.SrcAdd = m.mem.alloc<real>(NEQ * N);
  m.beta = m.mem.alloc<real>(NEQ * N);
  m.p = m.mem.alloc<real>(N);
  m.kk = m.mem.alloc<real>(N);
  m.R = m.mem.alloc<real>(N);
  m.CP = m.mem.alloc<real>(N);
  m.lam = m.mem.alloc<real>(N);
  m.mu = m.mem.alloc<real>(N);
  m.mu_t = m.mem.alloc<real>(N);
  m.lam_t = m.mem.alloc<real>(N);
  m.Diff = m.mem.alloc<real>(N);
  m.Y = m.mem.alloc<real>(NSPEC * N);
  m.l_min = m.mem.alloc<real>(N);
  m.y_plus = m.mem.alloc<real>(N);
  m.Re_local = m.mem.alloc<real>(N);
  m.BGX = m.mem.alloc<real>(N);
  m.BGY = m.mem.alloc<real>(N);
  m.Tf = m.mem.alloc<real>(N);
  m.Q_conv = m.mem.alloc<real>(N);
  m.grad = m.mem.alloc<real>(NGRAD * N);
  m.qdir = m.mem.alloc<real>(4 * N);
  m.CT = m.mem.alloc<u64>(N);
  m.TT = m.mem.alloc<u64>(N);
  m.nb = m.mem.alloc<uint8_t>(N);
  m.wslot = m.mem.alloc<int32_t>(N);
  h.allocate_mech(c);
  if (h.mech) {
    m.nsp = h.nsp;
    const long n = (long)m.nsp * N;
    m.mech = m.mem.alloc<MechData>(1);
    for (int b = 0; b < 2; b++) m.Ys[b] = m.mem.alloc<real>(n);
    m.As = m.mem.alloc<real>(n);
    m.Bs = m.mem.alloc<real>(n);
    m.Fs = m.mem.alloc<real>(n);
    m.betas = m.mem.alloc<real>(n);
    if (!h.dSdxs[0].empty())
      for (int b = 0; b < 2; b++) {
        m.dSdxs[b] = m.mem.alloc<real>(n);
        m.dSdys[b] = m.mem.alloc<real>(n);
      }
  }
  m.species = &m.mem.alloc<SpeciesDev>(1)->sp;   // (with its AirTable: air_table_of)
  m.scen = m.mem.alloc<ScenarioTables>(1);
  m.sc = m.mem.alloc<DevScalars>(1);
  HIP_CHECK(hipHostMalloc((void**)&m.sc_host, sizeof(DevScalars), hipHostMallocDefault));
  m.host_done = m.mem.alloc<unsigned>((DT_SHARDS + 1) * FX_DONE_STRIDE);
  {
    // any tile shape (lean_tj) covers >= LEAN_TILE_MIN_TJ cells per workgroup
    const long nb_tile = (long)(gi1 - gi0 + 1) * ((h.ny + LEAN_TILE_MIN_TJ - 1) / LEAN_TILE_MIN_TJ);
    m.max_partials = std::max((N + BLOCK - 1) / BLOCK, nb_tile) * (BLOCK / WAVE);
  }
  m.partials = m.mem.alloc<ResidualPack>(m.max_partials);
  m.res_out = m.mem.alloc<ResidualPack>(1);
  HIP_CHECK(hipHostMalloc((void**)&m.res_host, sizeof(ResidualPack), hipHostMallocDefault));
  m.halo_cap = (long)MAX_HALO_FIELDS * h.ny;
  for (int d = 0; d < 2; d++) {
    m.halo_send[d] = m.mem.alloc<real>(m.halo_cap);
    m.halo_recv[d] = m.mem.alloc<real>(m.halo_cap);
  }
  // hipMemset on device memory is asynchronous and runs on the null stream,
  // which does not order against the non-blocking solver stream: drain the
  // zero-fills before upload() copies the state in.
  HIP_CHECK(hipDeviceSynchronize());
  upload();
}

DeviceSolver::~DeviceSolver() {
  try {
    flush_pending();
  } catch (...) {
  }
  graph.reset();
  host_comm.reset();
  if (impl) {
    if (impl->stream) (void)hipStreamSynchronize(impl->stream);
    for (void* p : impl->p2p.opened) (void)hipIpcCloseMemHandle(p);
    if (impl->comm) ncclCommDestroy(impl->comm);
    if (impl->sc_host) (void)hipHostFree(impl->sc_host);
    if (impl->res_host) (void)hipHostFree(impl->res_host);
    if (impl->comm_stream) (void)hipStreamSynchronize(impl->comm_stream);
    if (impl->ev_edge) (void)hipEventDestroy(impl->ev_edge);
    if (impl->ev_halo) (void)hipEventDestroy(impl->ev_halo);
    for (hipEvent_t e : impl->lnm_ev)
      if (e) (void)hipEventDestroy(e);
    if (impl->comm_stream) (void)hipStreamDestroy(impl->comm_stream);
    if (impl->stream) (void)hipStreamDestroy(impl->stream);
  }
}

void* DeviceSolver::stream() const { return (void*)impl->stream; }

void DeviceSolver::upload() {
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  h.from_field(cs.J, gi0 - l_off);
  h.wall_slots(cs, gi0 - l_off, gi0, gi1);
  Impl& m = *impl;
  hipStream_t st = m.stream;
  const long N = h.N;
  if (!m.wall_own) {   // K10 buffers (sizes fixed by the grid's wall nodes)
    m.wall_own = m.mem.alloc<long>(h.wall_own.size());
    m.wall_uw = m.mem.alloc<real>(h.wall_own.size());
    m.wall_ok = m.mem.alloc<uint8_t>(h.wall_own.size());
    m.uw_all = m.mem.alloc<real>(cs.wall_nodes.size());
    m.uw_all_ok = m.mem.alloc<uint8_t>(cs.wall_nodes.size());
  }
  if (!h.wall_own.empty())
    HIP_CHECK(hipMemcpyAsync(m.wall_own, h.wall_own.data(), h.wall_own.size() * sizeof(long), hipMemcpyHostToDevice, st));
  auto cp = [&](void* d, const void* s, size_t bytes) { HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, st)); };
  const size_t EQB = NEQ * N * sizeof(real), SB = N * sizeof(real);
  for (int b = 0; b < 2; b++) {
    cp(m.S[b], h.S[0].data(), EQB);
    cp(m.A[b], h.A.data(), EQB);
    cp(m.B[b], h.B.data(), EQB);
    cp(m.dSdx[b], h.dSdx[0].data(), EQB);
    cp(m.dSdy[b], h.dSdy[0].data(), EQB);
    cp(m.U[b], h.U[0].data(), SB);
    cp(m.V[b], h.V[0].data(), SB);
    cp(m.Tg[b], h.Tg[0].data(), SB);
  }
  cp(m.F, h.F.data(), EQB);
  cp(m.Src, h.Src.data(), EQB);
  cp(m.SrcAdd, h.SrcAdd.data(), EQB);
  cp(m.beta, h.beta.data(), EQB);
  cp(m.p, h.p.data(), SB);
  cp(m.kk, h.kk.data(), SB);
  cp(m.R, h.R.data(), SB);
  cp(m.CP, h.CP.data(), SB);
  cp(m.lam, h.lam.data(), SB);
  cp(m.mu, h.mu.data(), SB);
  cp(m.mu_t, h.mu_t.data(), SB);
  cp(m.lam_t, h.lam_t.data(), SB);
  cp(m.Diff, h.Diff.data(), SB);
  cp(m.Y, h.Y.data(), NSPEC * SB);
  cp(m.l_min, h.l_min.data(), SB);
  cp(m.y_plus, h.y_plus.data(), SB);
  cp(m.Re_local, h.Re_local.data(), SB);
  cp(m.BGX, h.BGX.data(), SB);
  cp(m.BGY, h.BGY.data(), SB);
  cp(m.Tf, h.Tf.data(), SB);
  cp(m.Q_conv, h.Q_conv.data(), SB);
  cp(m.grad, h.grad.data(), NGRAD * SB);
  cp(m.CT, h.CT.data(), N * sizeof(u64));
  cp(m.TT, h.TT.data(), N * sizeof(u64));
  cp(m.nb, h.nb.data(), N);
  compute_generic_flags(cs, h, gi0 - l_off);
  cp(m.gf, h.gf.data(), N);
  chem_fast_ok = cs.cfg.mech_mode() && chem_fast_available(cs.cfg.mech->name) &&
                 mech_is_builtin(*cs.cfg.mech, cs.cfg.mech->name);
  chem_rtc_ok = false;
  chem_rtc_why.clear();
  if (cs.cfg.mech_mode() && (chem_kernel == 4 || (chem_kernel == 0 && !chem_fast_ok && chem_rtc)))
    chem_rtc_ok = chem_rtc_prepare(*cs.cfg.mech->data_ptr(), &chem_rtc_why);   // compile now, not in a step graph
  lean_ok = lean_eligible(cs, &lean_why);
  sk_mode = sk_eligible(cs, &sgl_why);
  sgl_ok = sk_mode != SK_GENERIC;
  {
    // lean N-S (lean_ns.hpp): laminar single gas, flat, adiabatic walls, no
    // volume sources, every non-solid node set (fluxes of skipped or unset
    // nodes are not recomputable), one strip (no 2-column halo)
    auto no = [&](const char* w) {
      lns_ok = false;
      lns_why = w;
    };
    lns_ok = true;
    lns_why.clear();
    // turbulence: one of k-eps (without Chien's model: it reads the previous
    // p), k-omega SST or Spalart-Allmaras, and no eddy-viscosity term in the
    // dt (the own-cell part of the next fill has no gradients)
    const u64 other_models = TCT_Prandtl_Model | TCT_Integral_Model | TCT_k_omega_Model | TCT_Baldwin_Lomax_Model |
                             TCT_nut_92_Model | TCT_Smagorinsky_Model;
    lns_turb = 2;
    u64 models = 0;
    if (sk_mode != SK_SGL && sk_mode != SK_SGT) no("not single-gas N-S");
    else if (!cs.cfg.isAdiabaticWall) no("wall heat transfer");
    else if (cs.cfg.WallBlendCells > 0) no("WallBlendCells (split path only)");
    else if ((gi0 > 0 && l_off < 2) || (gi1 < cs.J.nx && h.nx - l_off - (gi1 - gi0) < 2)) no("one ghost column");
    else if (sk_mode == SK_SGT && cs.cfg.ViscousCFL > 0) no("viscous CFL with eddy viscosity");
    else
      for (long q = 0; q < N && lns_ok; q++) {
        if (h.gf[q] & GF_SRC) no("volume sources");
        else if (!has_all(h.CT[q], CT_SOLID) && !has_all(h.CT[q], CT_NODE_IS_SET)) no("unset non-solid node");
        else if (h.TT[q] & other_models) no("turbulence model other than k-eps, SST or SA");
        else models |= h.TT[q] & (TCT_k_eps_Model | TCT_k_omega_SST_Model | TCT_Spalart_Allmaras_Model);
      }
    // one model per kernel (fill_node's turbulence set)
    if (lns_ok && models == TCT_k_omega_SST_Model) lns_turb = 3;
    else if (lns_ok && models == TCT_Spalart_Allmaras_Model) lns_turb = 4;
    else if (lns_ok && models != 0 && models != TCT_k_eps_Model) no("more than one turbulence model");
    else if (lns_ok && models == TCT_k_eps_Model && cs.cfg.TurbExtModel == TEM_k_eps_Chien) no("Chien k-eps");
    if (lns_ok) m.alloc_levels(N);
    if (m.CP2) {
      cp(m.CP2, h.CP.data(), SB);
      cp(m.mu2, h.mu.data(), SB);
      cp(m.lam2, h.lam.data(), SB);
      cp(m.kk2, h.kk.data(), SB);
      cp(m.mu_t2, h.mu_t.data(), SB);
    }
    lns_prev_mu_t = -1;
    lns_state = 0;
    cbuf = 0;
  }
  {
    // lean mechanism step (lean_mech.hpp): N-S, laminar or k-omega SST only
    // (SA / k-eps read values of the previous level before the state), no
    // eddy-viscosity or viscous CFL term in the dt (the state part has no
    // gradients), adiabatic walls, no volume sources, every non-solid node
    // set, one strip, <= LNM_NSB species
    auto no = [&](const char* w) {
      lnm_ok = false;
      lnm_why = w;
    };
    lnm_ok = true;
    lnm_why.clear();
    lnm_turb = 0;
    const u64 other_models = TCT_Prandtl_Model | TCT_Integral_Model | TCT_Spalart_Allmaras_Model |
                             TCT_k_omega_Model | TCT_k_eps_Model | TCT_Baldwin_Lomax_Model | TCT_nut_92_Model |
                             TCT_Smagorinsky_Model;
    if (!h.mech) no("not mechanism mode");
    else if (cs.cfg.ProblemType != SM_NS) no("not Navier-Stokes");
    else if (m.nsp > LNM_NSB || m.nsp < 2) no("species count outside the kernel's block");
    else if (!cs.cfg.isAdiabaticWall) no("wall heat transfer");
    else if (cs.cfg.WallBlendCells > 0) no("WallBlendCells (split path only)");
    else if ((gi0 > 0 && l_off < 2) || (gi1 < cs.J.nx && h.nx - l_off - (gi1 - gi0) < 2)) no("one ghost column");
    else if (cs.cfg.ViscousCFL > 0) no("viscous CFL");
    else if (h.ny < LNM_TILE) no("grid lower than one tile");
    else
      for (long q = 0; q < N && lnm_ok; q++) {
        if (h.gf[q] & GF_SRC) no("volume sources");
        else if (!has_all(h.CT[q], CT_SOLID) && !has_all(h.CT[q], CT_NODE_IS_SET)) no("unset non-solid node");
        else if (h.TT[q] & other_models) no("turbulence model other than k-omega SST");
        else if (has_all(h.TT[q], TCT_k_omega_SST_Model)) lnm_turb = 3;
      }
    if (lnm_ok) {
      m.alloc_levels(N);
      if (!m.p2) {
        m.p2 = m.mem.alloc<real>(N);
        m.Tst[0] = m.mem.alloc<real>(N);
        m.Tst[1] = m.mem.alloc<real>(N);
      }
      if (!m.chem_list) {
        m.chem_list = m.mem.alloc<int>(N);
        m.chem_count = m.mem.alloc<unsigned>(1);
      }
    }
  }
  lean_sg_ok = lean_ok && lean_single_gas(cs);
  any_cauchy_x = lean_any_cauchy_x(cs);
  lean_has_cauchy_x = lean_ok && any_cauchy_x;
  ghost_mode = -1;
  if (lean_ok) {
    lean_bytes = lean_flags(h, cs.cfg.ProblemType);
    if (!lean_plain)
      for (auto& b : lean_bytes) b &= (uint8_t)~LB_PLAIN;
    cp(m.lb, lean_bytes.data(), N);
  }
  lean_state = 0;
  cp(m.wslot, h.wslot.data(), N * sizeof(int32_t));
  {
    // the species pack and, rebuilt with every upload of it, its AirTable
    SpeciesDev& sd = m.species_host;
    sd.sp = cs.cfg.species;
    sd.air = air_table_build(sd.sp);
    cp(m.species, &sd, sizeof(SpeciesDev));
    air_table_mode = sd.air.mode;
  }
  if (h.mech) {
    h.mech_from_case(cs, gi0 - l_off);
    const size_t YB = (size_t)m.nsp * N * sizeof(real);
    cp(m.mech, h.mech, sizeof(MechData));
    for (int b = 0; b < 2; b++) cp(m.Ys[b], h.Ys[0].data(), YB);
    cp(m.As, h.As.data(), YB);
    cp(m.Bs, h.Bs.data(), YB);
    cp(m.Fs, h.Fs.data(), YB);
    cp(m.betas, h.betas.data(), YB);
    if (m.dSdxs[0])
      for (int b = 0; b < 2; b++) {
        cp(m.dSdxs[b], h.dSdxs[0].data(), YB);
        cp(m.dSdys[b], h.dSdys[0].data(), YB);
      }
  }
  scen_host.cfl = cs.cfg.CFL_Scenario.pack();
  scen_host.beta = cs.cfg.beta_Scenario.pack();
  scen_host.CFL = cs.cfg.CFL;
  scen_host.beta0 = cs.cfg.beta0;
  cp(m.scen, &scen_host, sizeof(ScenarioTables));
  DevScalars s0{};
  const double d0 = dt;
  const double one = 1.0;  // slot 1 accumulates step 0's min; slot 2 is reset by step 0
  unsigned long long b0, b1;
  std::memcpy(&b0, &d0, 8);
  std::memcpy(&b1, &one, 8);
  dt_set_host(s0, 0, b0);
  dt_set_host(s0, 1, b1);
  dt_set_host(s0, 2, b1);
  if (make_params(last_iter + iter).lag_dt) {
    // lagged dt: the first step runs with dt; slot 0's MIN stands for the
    // previous step's (the host's dt_lag, or dt before any step)
    s0.dt_lag[0] = b0;
    const double dl = dt_lag > 0 ? dt_lag : dt;
    unsigned long long bl;
    std::memcpy(&bl, &dl, 8);
    dt_set_host(s0, 0, bl);
  }
  s0.time_part = 0.0;
  s0.iter[0] = s0.iter[1] = s0.iter[2] = (double)(last_iter + iter);
  {
    const StepParams Pi = make_params(last_iter + iter);
    for (int q = 0; q < 3; q++) {
      s0.beta_min[q] = Pi.beta_min;
      s0.cfl_min[q] = Pi.CFL_min;
    }
  }
  time_offset = -cur_time_part;
  last_dev_time = 0.0;
  *m.sc_host = s0;
  cp(m.sc, m.sc_host, sizeof(DevScalars));
  m.sc_mirrored = false;
  // the accumulator's clock is time_part - t_off, the host's cur_time_part:
  // it goes on from the host's value across the restart of time_part, and no
  // sample is weighted across an upload
  // (the weights of the wall heat and the surface recorder likewise)
  const double st_clock[2] = {(double)cur_time_part, time_offset};
  static_assert(offsetof(StatsScalars, t_seen) + sizeof(double) == offsetof(StatsScalars, t_off), "adjacent");
  for (StatsScalars* t : tick_scalars()) cp(&t->t_seen, st_clock, sizeof st_clock);
  HIP_CHECK(hipStreamSynchronize(st));
  nstep = 0;
  abuf = 0;
  sbuf = 0;
  dsbuf = 0;
  pbuf = 0;
  plans_rebuild();   // (the records were replaced: the armed recorders' cells follow their flags)
}

std::vector<StatsScalars*> DeviceSolver::tick_scalars() const {
  std::vector<StatsScalars*> t;
  if (stats_armed) t.push_back(impl->stats.sc);
  if (wallq_armed) t.push_back(&impl->wallq.ring.sc->s);
  if (surf_armed) t.push_back(&impl->surf.ring.sc->s);
  if (frames_armed) t.push_back(&impl->frames.ring.sc->s);
  return t;
}

void DeviceSolver::set_lean_plain(bool on) {
  lean_plain = on;
  if (!lean_ok) return;
  std::vector<uint8_t> b = lean_flags(h, cs.cfg.ProblemType);
  if (!on)
    for (auto& x : b) x &= (uint8_t)~LB_PLAIN;
  lean_bytes = b;
  HIP_CHECK(hipMemcpyAsync(impl->lb, lean_bytes.data(), lean_bytes.size(), hipMemcpyHostToDevice, impl->stream));
  HIP_CHECK(hipStreamSynchronize(impl->stream));
}

void DeviceSolver::download(Field& J) {
  flush_pending();
  p2p_complete();
  HIP_CHECK(hipSetDevice(dev));
  Impl& m = *impl;
  if (lean_state) lean_materialize();
  if (lns_state) lns_materialize();
  hipStream_t st = m.stream;
  const long N = h.N;
  auto cp = [&](void* d, const void* s, size_t bytes) { HIP_CHECK(hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, st)); };
  const size_t EQB = NEQ * N * sizeof(real), SB = N * sizeof(real);
  cp(h.S[0].data(), m.S[sbuf], EQB);
  cp(h.A.data(), m.A[abuf], EQB);
  cp(h.B.data(), m.B[abuf], EQB);
  cp(h.dSdx[0].data(), m.dSdx[dsbuf], EQB);
  cp(h.dSdy[0].data(), m.dSdy[dsbuf], EQB);
  cp(h.U[0].data(), m.U[pbuf], SB);
  cp(h.V[0].data(), m.V[pbuf], SB);
  cp(h.Tg[0].data(), m.Tg[pbuf], SB);
  cp(h.F.data(), m.F, EQB);
  cp(h.Src.data(), m.Src, EQB);
  cp(h.SrcAdd.data(), m.SrcAdd, EQB);
  cp(h.beta.data(), m.beta, EQB);
  cp(h.p.data(), m.p, SB);
  cp(h.kk.data(), m.kk, SB);
  cp(h.R.data(), m.R, SB);
  cp(h.CP.data(), m.CP, SB);
  cp(h.lam.data(), m.lam, SB);
  cp(h.mu.data(), m.mu, SB);
  cp(h.mu_t.data(), m.mu_t, SB);
  cp(h.lam_t.data(), m.lam_t, SB);
  cp(h.Diff.data(), m.Diff, SB);
  cp(h.Y.data(), m.Y, NSPEC * SB);
  cp(h.y_plus.data(), m.y_plus, SB);
  cp(h.Re_local.data(), m.Re_local, SB);
  cp(h.Q_conv.data(), m.Q_conv, SB);
  cp(h.grad.data(), m.grad, NGRAD * SB);
  cp(h.CT.data(), m.CT, N * sizeof(u64));
  if (h.mech) cp(h.Ys[0].data(), m.Ys[sbuf], (size_t)m.nsp * N * sizeof(real));
  HIP_CHECK(hipStreamSynchronize(st));
  h.to_field(J, gi0 - l_off, l_off, l_off + (gi1 - gi0), 0, 0);
  h.mech_to_case(cs, gi0 - l_off, l_off, l_off + (gi1 - gi0), 0);
}

// The driver folded cur_time_part into global_time and restarts it at 0: the
// device's time_part restarts with it, so that the host's cur_time_part stays
// the plain sum of this cycle's dt -- bit for bit the CPU stepper's -- and not
// the difference of two running sums (one ulp off after the first cycle
// boundary).  Everything derived from time_part moves with it: the times the
// five rings and the peak-time planes store (host_time() converts those of
// earlier cycles as before) and the offsets of the four ticks' clocks (which
// go on unbroken).
// Always called right after sync_scalars(), with no step in between:
// last_dev_time is the device's time_part now.
void DeviceSolver::on_cycle_roll() {
  Impl& m = *impl;
  flush_pending();
  HIP_CHECK(hipSetDevice(dev));
  const double T = last_dev_time;
  const double zero = 0.0;
  HIP_CHECK(hipMemcpyAsync(&m.sc->time_part, &zero, sizeof zero, hipMemcpyHostToDevice, m.stream));
  // (a paused recorder's rows are not of the trial steps' clock: autotune() ends in upload())
  if (probes_live()) m.shift_times(m.ring.times, (size_t)m.ring.cap, T);
  if (loads_live()) m.shift_times(m.loads.times, (size_t)m.loads.cap, T);
  if (wallq_live()) m.shift_ring(m.wallq.ring, (size_t)wallq_plan.nentries(), T);
  if (surf_live()) m.shift_ring(m.surf.ring, surf_plan.nentries(), T);
  if (frames_live()) m.shift_ring(m.frames.ring, 0, T);   // (no statistics: the rows' times alone)
  for (StatsScalars* t : tick_scalars()) m.shift_clock(t, T);
  HIP_CHECK(hipStreamSynchronize(m.stream));
  m.sc_host->time_part = 0.0;
  time_offset = 0.0;
  last_dev_time = 0.0;
}

void DeviceSolver::poison_cell(int gi, int j) {
  flush_pending();
  Impl& m = *impl;
  if (lns_state) lns_materialize();
  const long idx = (long)(gi - gi0 + l_off) * h.ny + j;
  static const real bad = -1.0e30;
  HIP_CHECK(hipMemcpyAsync(m.S[sbuf] + (long)I_RHOE * h.N + idx, &bad, sizeof bad, hipMemcpyHostToDevice, m.stream));
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

// driver phases as roctx ranges (rocprofv3 --marker-trace)
void DeviceSolver::trace_push(const char* name) { roctxRangePush(name); }
void DeviceSolver::trace_pop() { roctxRangePop(); }

const char* DeviceSolver::halo_transport() const {
  const Impl& m = *impl;
  return m.nranks < 2 ? "none" : m.p2p.on ? "p2p" : m.local ? "local" : m.comm ? "rccl" : "none";
}

std::string DeviceSolver::profile_path_facts() const {
  auto quoted = [](const std::string& s) {
    std::string q = "\"";
    for (const char ch : s) {
      if (ch == '"' || ch == '\\') q += '\\';
      q += (unsigned char)ch < 0x20 ? ' ' : ch;
    }
    return q + "\"";
  };
  const TileLast& t = lean_tile_last;
  char b[1024];
  std::snprintf(b, sizeof b,
                "\"fp\": %d, \"sk_mode\": %d, \"split_mode\": %d, \"lean_ok\": %s, \"lean_sg_ok\": %s, \"lns_ok\": %s, \"lns_turb\": %d, "
                "\"lns_steps\": %ld, \"lnm_steps\": %ld, \"graph_captures\": %ld, \"graph_launches\": %ld, "
                "\"lean_tile_last\": {\"nt\": %d, \"cpt\": %d, \"TI\": %d, \"TJ\": %d, \"nbi\": %d, \"nbj\": %d, "
                "\"fx\": %d, \"var\": %d, \"seen\": %d, \"table\": %d}, ",
                (int)(8 * sizeof(real)), sk_mode, split_mode(), lean_ok ? "true" : "false", lean_sg_ok ? "true" : "false",
                lns_ok ? "true" : "false", lns_turb, lns_steps, lnm_steps, graph_captures, graph_launches, t.nt, t.cpt,
                t.TI, t.TJ, t.nbi, t.nbj, t.fx, t.var, t.seen, t.table);
  return std::string(b) + "\"lean_why\": " + quoted(lean_why) + ", \"lns_why\": " + quoted(lns_why) +
         ", \"transport\": " + quoted(halo_transport());
}

void DeviceSolver::sync_scalars() {
  flush_pending();
  p2p_complete();
  Impl& m = *impl;
  if (m.sc_mirrored) {
    // the last step wrote the mirror (host_tail).  It refreshes ONLY the dt
    // shards, dt_bits, dt_lag, time_part and neg_T of sc_host; the other
    // DevScalars fields there (iter, scenario beta / CFL, dt_val, hot counts)
    // are stale, so this function must read nothing else below this point
    // (hf2d_scalars_out refreshes the whole header).
  } else {
    hipLaunchKernelGGL(hf2d_scalars_out, dim3(1), dim3(WAVE), 0, m.stream, m.sc, m.sc_host, (int)(nstep % 3));
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipStreamSynchronize(m.stream));
  const int slot = nstep % 3;
  const unsigned long long db = dt_get_host(*m.sc_host, slot);
  if (make_params(last_iter + iter).lag_dt) {   // next step's dt, and the MIN it hands on
    std::memcpy(&dt, &m.sc_host->dt_lag[slot], 8);
    std::memcpy(&dt_lag, &db, 8);
  } else {
    std::memcpy(&dt, &db, 8);
  }
  cur_time_part = m.sc_host->time_part - time_offset;
  last_dev_time = m.sc_host->time_part;
  const int err = comm->allreduce_max_int(m.sc_host->neg_T);
  if (err & 2) {
    char b[256];
    std::snprintf(b, sizeof b, "ERROR: P2P halo exchange timed out (peer rank not responding) before iteration %ld",
                  last_iter + iter);
    throw std::runtime_error(b);
  }
  if (err & LNS_SKIP_ERR) {
    char b[256];
    std::snprintf(b, sizeof b, "ERROR: lean N-S step: FillNode2D skipped a node (rho = 0 or k < 1) before iteration %ld",
                  last_iter + iter);
    throw std::runtime_error(b);
  }
  if (err) {
    char b[256];
    std::snprintf(b, sizeof b, "ERROR: Computational unstability (Tg < 0) before iteration %ld", last_iter + iter);
    throw std::runtime_error(b);
  }
}

// ---------------------------------------------------------------------------
// Step graphs.  Plain steps (no residual pass, no host read-back) are queued
// and executed GRAPH_STEPS at a time as one captured hipGraph: every kernel
// argument is step-invariant over that window (dt, time and the scenario
// CFL/beta come from device memory; ping-pong parities repeat every 2 steps
// and dt slots every 3, so 6 steps bring both back), which removes the
// per-launch host cost that dominates small multi-GPU strips.  Any capture
// error disables graphs for the solver and the queue runs eagerly.
// ---------------------------------------------------------------------------
namespace {
constexpr int GRAPH_STEPS = 6;
// Everything that selects the kernels of a step besides the step parameters
// (DeviceSolver::mode_signature): a window replays only under the same one.
uint64_t graph_signature(const StepParams& P, uint64_t mode) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
  mix((uint64_t)P.fpa.is_mu_t);
  mix((uint64_t)P.fpa.is_init);
  mix((uint64_t)P.fpa.isSrcAdd);
  mix(mode);
  return h;
}
}  // namespace

void DeviceSolver::flush_pending() {
  if (pending.empty()) return;
  std::vector<StepParams> q;
  q.swap(pending);
  for (const StepParams& p : q) do_step_eager(p, false);
}

uint64_t DeviceSolver::mode_signature() const {
  // (the ping-pong parities too: a captured window bakes in the buffer
  // pointers of its first step, and a materialise + re-entry (split) step
  // flips only some of them, so a window cached before a download must not
  // replay after it -- it did, and the lean mechanism run then stepped on
  // the previous level's buffers from the first replayed window on)
  uint64_t h = 0;
  auto mix = [&](int f) { h = h * 1000003ull + (uint64_t)(f + 1); };
  // every knob a captured launch bakes in (the `graph` rows of device_knobs.hpp)
#define HF2D_KNOB_MIX(name, type, def, env, graph) \
  if (graph) mix((int)name);
  HF2D_DEVICE_KNOBS(HF2D_KNOB_MIX)
#undef HF2D_KNOB_MIX
  // and the state that is not a knob
  const int state[] = {lean_state, lns_state, sbuf, abuf, dsbuf, pbuf, cbuf, (int)(p2p_fuse && impl->p2p.on),
                       // (a window captured before an observer was armed has none of its launches,
                       // one captured before it was armed again, stopped, or its plan rebuilt by
                       // upload holds the previous arguments)
                       observers_gen};
  for (int f : state) mix(f);
  return h;
}

StepResult DeviceSolver::do_step(const StepParams& P0, bool want_res) {
  Impl& m = *impl;
  // (the in-process host transport synchronises on the host: eager only;
  // so does lnm_timing, which waits for each step's phase events)
  const bool plain = use_graph && !want_res && !step_outputs && !lnm_timing && (!m.local || m.p2p.on) &&
                     !(lean && lean_ok && lean_state == 0) &&
                     !(lns_state == 0 && lns_entry(P0));   // lean N-S entry step: eager
  if (!plain || (pending.empty() && nstep % GRAPH_STEPS != 0)) {
    flush_pending();
    return do_step_eager(P0, want_res);
  }
  pending.push_back(P0);
  if ((int)pending.size() == GRAPH_STEPS) run_graph();
  StepResult r;
  r.async = true;
  return r;
}

void DeviceSolver::run_graph() {
  Impl& m = *impl;
  m.sc_mirrored = false;
  const uint64_t mode = mode_signature();
  const uint64_t sig = graph_signature(pending[0], mode);
  bool same = true;
  for (const StepParams& p : pending) same = same && graph_signature(p, mode) == sig;
  if (!same) {
    flush_pending();
    return;
  }
  if (!graph) graph.reset(new GraphCache);
  if (graph->exec && graph->sig == sig) {
    if (graph->lns_pro && !lns_last_valid) {   // (the mailbox holds another exchange's layout)
      flush_pending();
      return;
    }
    if (!graph->lns_pro) p2p_complete();
    HIP_CHECK(hipGraphLaunch(graph->exec, m.stream));
    if (graph->lns_end) {
      m.lns_pend = graph->lns_end_list;
      lns_ghost_pending = lns_last_valid = true;
    }
    dt_word_valid = false;   // (conservative: the next eager step reads the shards too)
    {
      const TileLast prev = lean_tile_last;
      lean_tile_last = graph->tile_last;
      if (prev.nt == lean_tile_last.nt && prev.cpt == lean_tile_last.cpt) lean_tile_last.seen |= prev.seen;
    }
    nstep += GRAPH_STEPS;   // ping-pong parities are unchanged after an even number of steps
    pending.clear();
    graph_launches++;
    return;
  }
  // capture the window (host bookkeeping advances as in eager mode)
  const long nstep0 = nstep;
  const int ab = abuf, ds = dsbuf, pb = pbuf, sb = sbuf, ls = lean_state;
  std::vector<StepParams> q;
  q.swap(pending);
  hipGraph_t g = nullptr;
  // (a replayed window may follow any launch: its first step reads the shards)
  dt_word_valid = false;
  const bool s_pend = lns_ghost_pending, s_valid = lns_last_valid;
  const ColList s_list = m.lns_pend;
  bool first_pro = false;
  bool ok = hipStreamBeginCapture(m.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
  if (ok) {
    try {
      for (size_t k = 0; k < q.size(); k++) {
        lns_pro_uses = 0;
        do_step_eager(q[k], false);
        if (k == 0) first_pro = lns_pro_uses > 0;
      }
    } catch (const std::exception&) {
      ok = false;
    }
    hipGraph_t gg = nullptr;
    const bool ended = hipStreamEndCapture(m.stream, &gg) == hipSuccess;
    ok = ok && ended && gg != nullptr;
    if (gg && !ok) (void)hipGraphDestroy(gg);
    g = ok ? gg : nullptr;
  }
  hipGraphExec_t exec = nullptr;
  if (ok) ok = hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) == hipSuccess;
  if (g) (void)hipGraphDestroy(g);
  (void)hipGetLastError();
  // restore the bookkeeping and execute
  nstep = nstep0;
  abuf = ab;
  dsbuf = ds;
  pbuf = pb;
  sbuf = sb;
  lean_state = ls;
  if (!ok) {
    use_graph = false;   // eager from now on
    lns_ghost_pending = s_pend;   // (nothing of the capture ran)
    lns_last_valid = s_valid;
    m.lns_pend = s_list;
    for (const StepParams& p : q) do_step_eager(p, false);
    return;
  }
  if (graph->exec) (void)hipGraphExecDestroy(graph->exec);
  graph->exec = exec;
  graph->sig = sig;
  graph->lns_pro = first_pro;
  graph->lns_end = lns_ghost_pending && lns_last_valid;
  graph->lns_end_list = m.lns_pend;
  graph->tile_last = lean_tile_last;
  graph_captures++;
  HIP_CHECK(hipGraphLaunch(graph->exec, m.stream));
  nstep += GRAPH_STEPS;
  graph_launches++;
}

// The kernels that run a step with the (completed) parameters P.
DeviceSolver::StepPath DeviceSolver::step_path(const StepParams& P) const {
  if (P.sm != SM_NS) {
    if (lean && lean_ok) return lean_tile && lean_state == 1 && P.ny >= LEAN_TILE_MIN_TJ ? StepPath::Tile : StepPath::LeanFlat;
    if (fused && !impl->mech) return StepPath::FusedEuler;
  }
  return lnm_step_ok(P) ? StepPath::LeanMech : lns_step_ok(P) ? StepPath::LeanNs : StepPath::Split;
}

StepResult DeviceSolver::do_step_eager(const StepParams& P0, bool want_res) {
  Impl& m = *impl;
  hipStream_t st = m.stream;
  m.sc_mirrored = false;
  StepCtx c{P0, want_res};
  StepParams& P = c.P;
  P.nx = h.nx;
  P.ny = h.ny;
  P.i0 = l_off;
  P.i1 = l_off + (gi1 - gi0);
  P.gx0 = gi0 - l_off;
  P.do_residual = want_res ? 1 : 0;
  P.species = m.species;
  P.scen = m.scen;
  c.c0 = (long)P.i0 * P.ny;
  c.c1 = (long)P.i1 * P.ny;
  c.nblk = (unsigned)((c.c1 - c.c0 + BLOCK - 1) / BLOCK);
  c.slot = nstep % 3;
  c.slot_next = (nstep + 1) % 3;
  c.serial = cs.cfg.semantics == Semantics::SERIAL ? 1 : 0;
  // the slot's word holds the MIN only right after a folding tile launch
  c.dt_word_ok = dt_word_valid;
  dt_word_valid = false;
  // the mailbox holds a fused lean N-S step's halo (list m.lns_pend) only
  // right after such a step (every other step or exchange publishes another
  // layout or nothing)
  lns_prev_valid = lns_last_valid;
  lns_last_valid = false;
  c.tile_prev = lean_tile_last;
  lean_tile_last = TileLast{};
  const StepPath path = step_path(P);
  // the ghost columns and dt of earlier fused steps, for every consumer but
  // the fused kernels themselves (the tile kernel reads the mailbox; a fused
  // lean N-S / mechanism step unpacks the previous fused step's halo itself)
  const bool lns_fx_next = (path == StepPath::LeanMech || path == StepPath::LeanNs) && lns_state == 1 &&
                           lean_state == 0 && m.p2p.on && p2p_fuse && m.nranks > 1;
  if (path != StepPath::Tile) p2p_complete(lns_fx_next);
  StepDone done{};
  switch (path) {
    case StepPath::Tile: done = step_tile(c); break;
    case StepPath::LeanFlat: done = step_lean_flat(c); break;
    case StepPath::FusedEuler: done = step_fused_euler(c); break;
    case StepPath::LeanMech: done = lnm_step(c); break;
    case StepPath::LeanNs: done = step_lean_ns(c); break;
    case StepPath::Split:
      if (lean_state) lean_materialize();
      if (lns_state) lns_materialize();
      done = step_split(c, false);
      break;
  }
  // new-state halo + global dt (MIN over ranks into the next slot), unless
  // the step exchanged them itself (fused into its kernel, or overlapped
  // with its interior tiles)
  if (!done.exchanged && (m.comm || m.local || m.p2p.on) && m.nranks > 1)
    exchange(lns_state ? CpuSolver::HALO_LNS : lean_state ? CpuSolver::HALO_LEAN : CpuSolver::HALO_STATE, c.slot_next);
  if (!cs.cfg.isAdiabaticWall) wall_heat(c);
  if (probes_live() || stats_live() || loads_live() || wallq_live() || surf_live() || frames_live()) {
    const PostStep v = post_step(c.slot, c.slot_next);
    if (probes_live()) launch_probe_record(P, v);
    if (stats_live()) launch_stats(P, v);
    if (loads_live()) launch_loads(P, v);
    if (wallq_live()) launch_wall_heat(P, v);
    if (surf_live()) launch_surface(P, v);
    if (frames_live()) launch_frames(P, v);
  }
  nstep++;
  lns_prev_mu_t = P.fpa.is_mu_t;
  StepResult r;
  r.async = true;
  if (want_res) {
    hipLaunchKernelGGL(hf2d_reduce_residual, dim3(1), dim3(BLOCK), 0, st, m.partials,
                       (long)done.nres * done.nres_waves, m.res_out);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(m.res_host, m.res_out, sizeof(ResidualPack), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    r.res = *m.res_host;
    r.have_residual = true;
  }
  return r;
}

void DeviceSolver::synchronize() {
  flush_pending();
  HIP_CHECK(hipStreamSynchronize(impl->stream));
}

// ThreadBlockSize = 0 ("auto-calibrate", UG p.20): time the lean tile
// kernel's geometry choices (cells per thread, tile height) on this device
// and strip, keep the fastest.  Every candidate computes the same bits; the
// state (device arrays and host bookkeeping) is restored afterwards, so the
// run is unaffected apart from its speed.  Only before the first step.
std::string DeviceSolver::autotune(int steps) {
  // inviscid lean tile: cells per thread x tile height; lean N-S tile (one
  // cell per thread): tile height (resonator 2000x200: 92 us at the
  // heuristic height, 87 us at 16 rows)
  const bool ns = cs.cfg.ProblemType == SM_NS;
  if (nstep != 0 || iter != 0) return "";
  // mechanism mode: the lean mechanism tile's width (16 x 16: the ring is a
  // second fill on one wavefront; 12 x 16: one fill per thread)
  const bool mech = ns && lean_mech && lnm_ok && cs.cfg.mech_mode();
  if (ns ? !((lean_ns && lns_ok) || mech) : !(lean_ok && lean_tile)) return "";
  flush_pending();
  const real s_dt = dt, s_dtr = dt_running, s_cur = cur_time_part, s_gt = cs.global_time, s_lag = dt_lag;
  const long s_iter = iter, s_last = last_iter;
  const int s_cycle = cycle;
  const bool s_src = isSrcAdd, s_out = step_outputs;
  const ResidualSummary s_res = last_res;
  const bool s_resv = last_res_valid;
  observers_paused = true;   // the trial steps are not the run's: the armed observers sit them out
  struct Cand {
    int cpt, tj, nt, wgcu = 0;
  };
  std::vector<Cand> cands;
  for (int cpt : {2, 1}) {
    if (ns && cpt == 2) continue;
    if (mech) break;
    for (int tj : {0, 10, 12, 14, 16, 20, 25, 32, 40, 50, 64})
      if ((tj == 0 || tj <= h.ny) && (ns ? tj <= 40 : (tj == 0 || tj >= 16))) cands.push_back({cpt, tj, BLOCK});
  }
  if (mech)   // (Cand::tj carries the tile width here)
    for (int ti : {LNM_TILE, 12}) cands.push_back({1, ti, BLOCK});
  // small workgroups (single-gas inviscid): the geometries of the narrow
  // strips of a multi-GPU run, where 256-thread tiles leave CUs idle
  if (!ns && lean_sg && lean_sg_ok)
    for (int nt : {128, 64})
      for (int cpt : {1, 2})
        for (int tj : {0, 8, 16, 32, 64})
          if (tj <= nt && (tj == 0 || tj <= h.ny)) cands.push_back({cpt, tj, nt});
  double best = 1e30;
  Cand win = mech ? Cand{1, lnm_ti, BLOCK} : Cand{lean_cpt, lean_tj, lean_nt, lean_wgcu};
  char b[160];
  std::string log;
  // same work per candidate whatever the grid (~50 M cell-steps): big grids get fewer steps
  const long cells = std::max(1L, (long)(gi1 - gi0) * h.ny);
  steps = (int)std::max(12L, std::min((long)steps, 50000000L / cells));
  // second stage (inviscid): resident workgroups per CU for the winning
  // geometry (through the LDS request).  Fewer resident workgroups than
  // tiles make later dispatch rounds stage their tiles while earlier ones
  // compute instead of every workgroup loading, then computing, at once.
  bool stage2 = ns;
  for (size_t ci = 0; ci < cands.size(); ci++) {
    const Cand c = cands[ci];
    if (mech) {
      lnm_ti = c.tj;
    } else {
      lean_cpt = c.cpt;
      lean_tj = c.tj;
      lean_nt = c.nt;
      lean_wgcu = c.wgcu;
    }
    graph.reset();   // the state just keeps marching; it is restored once at the end
    double us = 1e30;
    try {
      run_steps(12);   // (first candidate: first lean step) + graph capture
      synchronize();
      for (int rep = 0; rep < 2; rep++) {   // best of two: the candidates differ by a few %
        const auto t0 = std::chrono::steady_clock::now();
        run_steps(steps);
        synchronize();
        us = std::min(us, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / steps * 1e6);
      }
    } catch (const std::exception& e) {   // e.g. the transient went unstable: stop tuning, keep the best so far
      log += std::string("stopped: ") + e.what() + "; ";
      break;
    }
    if (mech)
      std::snprintf(b, sizeof b, "lnm ti=%d %.2f us; ", c.tj, us);
    else if (c.wgcu)
      std::snprintf(b, sizeof b, "wgcu=%d %.2f us; ", c.wgcu, us);
    else if (c.nt == BLOCK)
      std::snprintf(b, sizeof b, "cpt=%d tj=%d %.2f us; ", c.cpt, c.tj, us);
    else
      std::snprintf(b, sizeof b, "nt=%d cpt=%d tj=%d %.2f us; ", c.nt, c.cpt, c.tj, us);
    log += b;
    if (us < best) {
      best = us;
      win = c;
    }
    if (!stage2 && ci + 1 == cands.size()) {
      stage2 = true;
      for (int w : {2, 3, 4, 6, 8, 12, 16}) {
        if (w * (win.nt / WAVE) > 32) break;   // (32 waves per CU)
        Cand c2 = win;
        c2.wgcu = w;
        cands.push_back(c2);
      }
    }
  }
  if (mech) {
    lnm_ti = win.tj;
  } else {
    lean_cpt = win.cpt;
    lean_tj = win.tj;
    lean_nt = win.nt;
    lean_wgcu = win.wgcu;
  }
  // step graphs on or off for the winning geometry: replaying the 6-step
  // graph costs ~1 us per step more than eager launches on the 2000 x 200
  // headline grid (28.5 vs 27.5 us/step over 20-step calls, 1x MI355X,
  // tools/launch_overhead.py) but saves host launch time on small grids
  if (use_graph) {
    double g_us[2] = {1e30, 1e30};
    for (int g : {1, 0}) {
      use_graph = g == 1;
      graph.reset();
      try {
        run_steps(12);
        synchronize();
        for (int rep = 0; rep < 2; rep++) {
          const auto t0 = std::chrono::steady_clock::now();
          run_steps(steps);
          synchronize();
          g_us[g] = std::min(g_us[g],
                             std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / steps * 1e6);
        }
      } catch (const std::exception& e) {
        log += std::string("stopped: ") + e.what() + "; ";
        break;
      }
    }
    use_graph = g_us[1] <= g_us[0];
    std::snprintf(b, sizeof b, "graphs on %.2f us, off %.2f us; ", g_us[1], g_us[0]);
    log += b;
  }
  graph.reset();
  dt = s_dt;
  dt_running = s_dtr;
  dt_lag = s_lag;
  cur_time_part = s_cur;
  cs.global_time = s_gt;
  iter = s_iter;
  last_iter = s_last;
  cycle = s_cycle;
  isSrcAdd = s_src;
  step_outputs = s_out;
  last_res = s_res;
  last_res_valid = s_resv;
  observers_paused = false;
  upload();   // device scalars from the restored host state
  graph_launches = 0;
  lns_steps = lnm_steps = 0;   // (the tuning steps do not count as the run's)
  if (mech)
    std::snprintf(b, sizeof b, "best lnm ti=%d graphs=%d (%.2f us/step)", win.tj, (int)use_graph, best);
  else
    std::snprintf(b, sizeof b, "best nt=%d cpt=%d tj=%d wgcu=%d graphs=%d (%.2f us/step)", win.nt, win.cpt, win.tj,
                  win.wgcu, (int)use_graph, best);
  return log + b;
}

std::unique_ptr<SolverBase> make_gpu_solver(Case& cs, int device) {
  return std::unique_ptr<SolverBase>(new DeviceSolver(cs, device < 0 ? 0 : device));
}

// Strip rank of the native multi-process CLI (hf2d_main.cpp).  `boot` is the
// host communicator (TCP): it carries the driver's host reductions and the
// p2p bootstrap -- every rank exports its xGMI mailbox descriptor, the
// descriptors are all-gathered and imported, one poisoned full-state exchange
// is checksummed on every rank (p2p_probe), and the ranks agree on the
// result.  If any rank fails (or transport "rccl" is asked for), the RCCL
// unique id travels through `boot` and every rank uses grouped RCCL
// send/recv on the solver stream instead.  `used` reports the transport.
std::unique_ptr<SolverBase> make_gpu_strip_solver(Case& cs, int device, int gi0, int gi1, Comm& boot,
                                                  const std::string& transport, std::string& used) {
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  // more local ranks than GPUs (tests on a one-GPU box): ranks share devices
  if (device >= ndev && ndev > 0) device %= ndev;
  std::unique_ptr<DeviceSolver> s(new DeviceSolver(cs, device < 0 ? 0 : device, gi0, gi1));
  used = "none";
  if (cs.cfg.ThreadBlockSize == 0 && s->autotune_enabled) s->autotune();
  if (boot.size() == 1) return std::unique_ptr<SolverBase>(s.release());
  const int r = boot.rank(), n = boot.size();
  auto use_rccl = [&] {
    const std::string uid = boot.allgather_bytes(r == 0 ? DeviceSolver::nccl_unique_id() : std::string())[0];
    s->init_comm(uid, r, n);
    used = "rccl";
  };
  if (transport != "p2p") {
    use_rccl();
    return std::unique_ptr<SolverBase>(s.release());
  }
  // host-side reductions of the driver (output steps) over the bootstrap
  // communicator; the halos and the per-step dt MIN go through the mailboxes
  s->comm = &boot;
  std::string desc, why;
  int bad = 0;
  try {
    desc = s->p2p_export(r, n);
  } catch (const std::exception& e) {
    bad = 1;
    why = e.what();
  }
  const std::vector<std::string> descs = boot.allgather_bytes(bad ? std::string() : desc);
  for (const std::string& d : descs) bad |= d.empty() ? 1 : 0;
  if (!bad) {
    try {
      s->p2p_import(descs);
    } catch (const std::exception& e) {
      bad = 1;
      why = e.what();
    }
  }
  if (boot.allreduce_max_int(bad) == 0) {
    // self-validation: one poisoned full-state exchange, checksummed
    const std::vector<std::string> probes = boot.allgather_bytes(s->p2p_probe());
    if (!DeviceSolver::p2p_probe_ok(probes, r, &why)) bad = 1;
  } else {
    bad = 1;
  }
  if (boot.allreduce_max_int(bad) == 0) {
    used = "p2p";
    s->p2p_fuse = s->p2p_fuse_wanted;
  } else {
    use_rccl();
    s->p2p_fallback();
    if (!why.empty()) std::fprintf(stderr, "[hf2d rank %d] p2p transport unavailable (%s); using RCCL\n", r, why.c_str());
  }
  return std::unique_ptr<SolverBase>(s.release());
}

}  // namespace hf2d
