// The N-S and split steps: the split predict / fill step of every N-S, mechanism
// and generic case with the fused Euler step, generic kinetics, wall heat and y+;
// the lean single-gas N-S tile step (lean_ns.hpp); the lean mechanism tile step
// (lean_mech.hpp).  Each section holds its kernels, their tables and the members
// that launch them.  The three families are one translation unit because their
// kernels share the fill (fill_compute / fill_node): what the compiler's
// interprocedural passes see of that code's other callers decides the register
// allocation of the fills and of hf2d_fused_euler (243 VGPRs and two waves per
// SIMD here, 260 registers and one wave compiled apart; profiles/split_units_ab.md).

#include "device_impl.hpp"
#include "lean_mech.hpp"

namespace hf2d {

// ---------------------------------------------------------------------------
// Split predict / fill step, fused Euler step, generic kinetics, wall heat, y+
// ---------------------------------------------------------------------------
// Split kernels (one cell per thread, x-major): logical block of this
// workgroup.  A column of a tall grid spans a few blocks, so the left/right
// neighbour reads of the round-robin order land on another XCD's L2; with
// StepParams::xcd the blocks of an XCD form one contiguous column range.
__device__ inline unsigned split_block(const StepParams& P) {
  return P.xcd ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
}

template <bool RES, int MODE = SK_GENERIC>
__global__ __launch_bounds__(BLOCK) void hf2d_predict(StepParams P, SoA in, SoA out, long c0, long c1,
                                                       DevScalars* sc, int slot, int slot_next, int serial,
                                                       ResidualPack* partials) {
  apply_dt(P, sc, slot);
  const unsigned blk = split_block(P);
  const long g = (long)blk * BLOCK + threadIdx.x;
  if (g == 0) {
    step_head(P, sc, slot, slot_next, P.dt);
    sc->dt_val[slot] = P.dt;
    sc->hot_cnt[slot_next] = 0;
  }
  const long c = c0 + g;
  ResidualPack r;
  if (RES) {
    residual_reset(r);
#pragma unroll
    for (int k = 0; k < NEQ; k++) r.eq[k].i = r.eq[k].j = -1;
  }
  if (c < c1) {
    const auto [i, j] = cell_ij(c, P.ny);
    predict_cell_t<RES, MODE>(P, in, out, i, j, r);
  }
  if (RES) residual_publish<BLOCK>(r, partials, blk);
}

template <int MODE, int NSB, bool LAZY = false>
__device__ __forceinline__ void fill_body(StepParams& P, const SoA& sin, const SoA& pold, const SoA& out, long c0,
                                          long c1, DevScalars* sc, int slot, int slot_next, int serial,
                                          int store_grad);

template <int MODE = SK_GENERIC, int NSB = 1>
__global__ __launch_bounds__(BLOCK) void hf2d_fill(StepParams P, SoA sin, SoA pold, SoA out, long c0, long c1,
                                                    DevScalars* sc, int slot, int slot_next, int serial,
                                                    int store_grad) {
  fill_body<MODE, NSB>(P, sin, pold, out, c0, c1, sc, slot, slot_next, serial, store_grad);
}

// The same fill with a register budget of OCC waves per SIMD (the split N-S
// fills compile to 165-255 VGPRs, i.e. 1-3 waves; DeviceSolver::fill_occ)
template <int MODE, int NSB, int OCC, bool LAZY = false>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(OCC))) void hf2d_fill_occ(
    StepParams P, SoA sin, SoA pold, SoA out, long c0, long c1, DevScalars* sc, int slot, int slot_next, int serial,
    int store_grad) {
  fill_body<MODE, NSB, LAZY>(P, sin, pold, out, c0, c1, sc, slot, slot_next, serial, store_grad);
}

template <int MODE, int NSB, bool LAZY>
__device__ __forceinline__ void fill_body(StepParams& P, const SoA& sin, const SoA& pold, const SoA& out, long c0,
                                          long c1, DevScalars* sc, int slot, int slot_next, int serial,
                                          int store_grad) {
  apply_dt(P, sc, slot);
  const long c = c0 + (long)split_block(P) * BLOCK + threadIdx.x;
  double dtl = 1.0;
  int neg = 0;
  if (c < c1) {
    const auto [i, j] = cell_ij(c, P.ny);
    dtl = fill_cell<MODE, NSB, LAZY>(P, sin, pold, out, i, j, &neg, store_grad != 0);
  }
  const double* sdt = block_dt_stage<BLOCK>(dtl);
  if (neg) atomicOr(&sc->neg_T, 1);
  __syncthreads();
  // (slot_next < 0: lean N-S materialize)
  if (threadIdx.x == 0) block_dt_commit<BLOCK>(sdt, sc, slot_next, serial, P.dt, slot_next >= 0);
}

// Mechanism mode, operator-split kinetics (runtime mechanism data; the
// per-cell point-implicit integrator of mechanism.hpp): predicted species
// mid.Ys -> out.Ys over the step's dt at constant rho and e.
template <int NSB>
__global__ __launch_bounds__(BLOCK) void hf2d_chem_generic(StepParams P, SoA mid, SoA out, const real* Tprev, long c0,
                                                            long c1, DevScalars* sc, int slot) {
  apply_dt(P, sc, slot);
  const long c = c0 + (long)blockIdx.x * BLOCK + threadIdx.x;
  if (c < c1) {
    const auto [i, j] = cell_ij(c, P.ny);
    mech_chem_soa_cell<NSB>(P, mid, out, Tprev, i, j);
  }
}

// Euler: no gradients, so the fill of a cell depends only on its own
// predicted state and the predictor and fill run in one sweep.  A and B are
// ping-ponged (neighbours read the old fluxes).
template <bool RES>
__global__ __launch_bounds__(BLOCK) void hf2d_fused_euler(StepParams P, SoA in, SoA mid, SoA out, long c0, long c1,
                                                           DevScalars* sc, int slot, int slot_next, int serial,
                                                           ResidualPack* partials) {
  apply_dt(P, sc, slot);
  const long g = (long)blockIdx.x * BLOCK + threadIdx.x;
  if (g == 0) step_head(P, sc, slot, slot_next, P.dt);
  const long c = c0 + g;
  ResidualPack r;
  if (RES) {
    residual_reset(r);
#pragma unroll
    for (int k = 0; k < NEQ; k++) r.eq[k].i = r.eq[k].j = -1;
  }
  double dtl = 1.0;
  int neg = 0;
  if (c < c1) {
    const auto [i, j] = cell_ij(c, P.ny);
    predict_cell_t<RES>(P, in, mid, i, j, r);
    dtl = fill_cell(P, mid, mid, out, i, j, &neg, false);
  }
  if (RES) residual_publish<BLOCK>(r, partials, blockIdx.x);
  for (int off = 1; off < WAVE; off <<= 1) dtl = fmin(dtl, __shfl_xor(dtl, off, WAVE));
  __shared__ double sdt[BLOCK / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) sdt[threadIdx.x / WAVE] = dtl;
  if (neg) atomicOr(&sc->neg_T, 1);
  __syncthreads();
  // (block_dt_stage / block_dt_commit written out, with a test that is dead here -- the one launch
  // passes (nstep + 1) % 3: either change moves this kernel's spills, profiles/step_epilogue_ab.md)
  if (threadIdx.x == 0) {
    double m = sdt[0];
    for (int q = 1; q < BLOCK / WAVE; q++) m = fmin(m, sdt[q]);
    if (serial) m = fmin(m, P.dt);  // serial build: dt is a running minimum
    if (slot_next >= 0) dt_min(sc, slot_next, m);   // < 0: lean N-S materialize
  }
}

__global__ __launch_bounds__(BLOCK) void hf2d_wall_solid(StepParams P, SoA s, real* qdir, long c0, long c1) {
  const long c = c0 + (long)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= c1) return;
  const auto [i, j] = cell_ij(c, P.ny);
  wall_heat_solid_cell(P, s, qdir, i, j);
}

__global__ __launch_bounds__(BLOCK) void hf2d_wall_wall(StepParams P, SoA s, const real* qdir, long c0, long c1,
                                                         const DevScalars* sc, int slot) {
  apply_dt(P, sc, slot);
  const long c = c0 + (long)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= c1) return;
  const auto [i, j] = cell_ij(c, P.ny);
  wall_heat_wall_cell(P, s, qdir, i, j);
}

// K10 in two passes: friction velocity of the wall nodes this strip owns
// (merged over the strips on the host), then y+ of every owned cell
__global__ __launch_bounds__(BLOCK) void hf2d_wall_uw(SoA s, const long* own, int n, real* uw, uint8_t* ok) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= n) return;
  const long w = own[k];
  const bool g = is_wall_gas(s.CT[w]);
  ok[k] = g ? 1 : 0;
  uw[k] = g ? wall_friction_velocity(s, w) : 0.;
}
__global__ __launch_bounds__(BLOCK) void hf2d_yplus(SoA s, long c0, long c1, const real* uw, const uint8_t* ok) {
  const long c = c0 + (long)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= c1) return;
  y_plus_apply(s, c, uw, ok);
}

using PredictK = void (*)(StepParams, SoA, SoA, long, long, DevScalars*, int, int, int, ResidualPack*);
// [residual][SK_* mode]
static const PredictK kPredict[2][4] = {
    {hf2d_predict<false, SK_GENERIC>, hf2d_predict<false, SK_SGL>, hf2d_predict<false, SK_SGT>,
     hf2d_predict<false, SK_MECH>},
    {hf2d_predict<true, SK_GENERIC>, hf2d_predict<true, SK_SGL>, hf2d_predict<true, SK_SGT>,
     hf2d_predict<true, SK_MECH>}};

using FillK = void (*)(StepParams, SoA, SoA, SoA, long, long, DevScalars*, int, int, int, int);
// register-budget slot of a fill: compiler default, 2, 3, 4 waves per SIMD
inline int occ_slot(int occ) { return occ == 2 ? 1 : occ == 3 ? 2 : occ == 4 ? 3 : 0; }
// [SK_* mode][occ_slot] (mechanism: the 9-species block)
static const FillK kFill[4][4] = {
    {hf2d_fill<SK_GENERIC>, hf2d_fill<SK_GENERIC>, hf2d_fill<SK_GENERIC>, hf2d_fill<SK_GENERIC>},
    {hf2d_fill<SK_SGL, 1>, hf2d_fill_occ<SK_SGL, 1, 2>, hf2d_fill_occ<SK_SGL, 1, 3>, hf2d_fill_occ<SK_SGL, 1, 4>},
    {hf2d_fill<SK_SGT, 1>, hf2d_fill_occ<SK_SGT, 1, 2>, hf2d_fill_occ<SK_SGT, 1, 3>, hf2d_fill_occ<SK_SGT, 1, 4>},
    {hf2d_fill<SK_MECH, 9>, hf2d_fill_occ<SK_MECH, 9, 2>, hf2d_fill_occ<SK_MECH, 9, 3>, hf2d_fill_occ<SK_MECH, 9, 4>}};

// Split predict + fill step (every N-S / mechanism / generic case).
DeviceSolver::StepDone DeviceSolver::step_split(const StepCtx& c, bool to_lns) {
  StepParams P = c.P;
  Impl& m = *impl;
  hipStream_t st = m.stream;
  const bool want_res = c.want_res;
  const int slot = c.slot, slot_next = c.slot_next, serial = c.serial;
  const unsigned nblk = c.nblk;
  const long c0 = c.c0, c1 = c.c1;
    SoA in = m.view(h, sbuf, abuf, dsbuf, pbuf);
    SoA mid = m.view(h, 1 - sbuf, abuf, 1 - dsbuf, pbuf);
    // single-gas N-S: only the live equations and fields move (SK_SGL/SK_SGT);
    // mechanism mode: SK_MECH (Euler and N-S)
    const int mode = m.mech ? SK_MECH : (P.sm == SM_NS && sgl) ? sk_mode : SK_GENERIC;
    // the ghost columns hold the lean N-S / mechanism representation (the
    // record was materialised): the split step's halo first
    if (ghost_stale) exchange(CpuSolver::HALO_STATE);
    // the ghost columns were last exchanged for a single-gas specialisation
    // and this step is generic (sgl switched off): refresh them in full first
    if (ghost_mode >= 0 && ghost_mode != SK_GENERIC && mode == SK_GENERIC)
      exchange(CpuSolver::HALO_STATE, -1, nullptr, true);
    // XCD-aware order: split Step 63.8 -> 59.2 us, resonator 117.7 -> 107.8 us
    // on 1x MI355X; the mechanism pair is 2 % slower with it (1.767 vs 1.800 ms)
    P.xcd = (split_xcd && (mode != SK_MECH || split_xcd_mech)) ? 1 : 0;
    hipLaunchKernelGGL(kPredict[want_res][mode], dim3(nblk), dim3(BLOCK), 0, st, P, in, mid, c0, c1, m.sc, slot,
                       slot_next, serial, m.partials);
    HIP_CHECK(hipGetLastError());
    const bool multi = (m.comm || m.local || m.p2p.on) && m.nranks > 1;
    if (P.sm == SM_NS) exchange(CpuSolver::HALO_MID);
    SoA sin = m.view(h, 1 - sbuf, abuf, 1 - dsbuf, pbuf);
    SoA out = m.view(h, sbuf, abuf, 1 - dsbuf, 1 - pbuf);
    if (to_lns && mode == SK_MECH) {
      // entering the lean mechanism path: transport of level n+1 into the
      // second buffers (level n stays for G_{n+1}); the state (T, p, Cp, k)
      // of level n+1 is read from the generic arrays (T copied to Tst[0])
      out.mu = m.mu2;
      out.lam = m.lam2;
      out.mu_t = m.mu_t2;
    } else if (to_lns) {   // entering the lean N-S path: level n+1 into the second buffers
      out.CP = m.CP2;
      out.mu = m.mu2;
      out.lam = m.lam2;
      out.kk = m.kk2;
      out.mu_t = m.mu_t2;
    }
    if (mode == SK_MECH) {
      // operator-split kinetics: Ys[1-sbuf] -> Ys[sbuf]; N-S strips also react
      // their ghost columns (exchanged above; same inputs as on the owner)
      const bool ghosts = multi && P.sm == SM_NS;
      const long k0 = ghosts ? c0 - (c0 > 0 ? h.ny : 0) : c0;
      const long k1 = ghosts ? c1 + (c1 < h.N ? h.ny : 0) : c1;
      const unsigned nbk = (unsigned)((k1 - k0 + BLOCK - 1) / BLOCK);
      launch_chem(P, sin, out, k0, k1, nbk, slot);
      m.mech_view(sin, sbuf, 1 - dsbuf);   // the fill reads the post-chemistry species
    }
    // SGL: gradients / Diff only when the host reads the record (or y+ follows)
    // (or the armed load recorder folds wall friction after every step: stores only, same values)
    const int sg_out = (step_outputs || want_res || friction_recorded()) ? 1 : 0;
    // SGT / mechanism: the gradients an active N-S cell stores are recomputed
    // by its next fill before any use (fill_compute), so between outputs
    // (and the wall friction velocities of the cycle end, an output step) they
    // are dead stores: 80 B/cell (HF2D_GRAD_EVERY=1 stores them every step)
    const int tg_out = grad_every ? 1 : sg_out;
    // register budget: measured on 1x MI355X (tools/fill_occ_sweep.sh): the
    // mechanism fill is 10 % faster at 2 waves/SIMD (256 VGPRs, a few spills)
    // than at the compiler's 1; SGL / SGT are fastest at the default
    const int focc = fill_occ >= 0 ? fill_occ : (mode == SK_MECH ? 2 : 0);
    FillK fk;
    int store = 1;
    if (mode == SK_MECH) {
      store = tg_out;
      fk = m.nsp > 9 ? hf2d_fill<SK_MECH, MECH_MAXSP>
                     : (mech_lazy && focc == 2) ? hf2d_fill_occ<SK_MECH, 9, 2, true> : kFill[SK_MECH][occ_slot(focc)];
    } else {
      store = mode == SK_SGL ? sg_out : mode == SK_SGT ? tg_out : 1;
      fk = kFill[mode][mode == SK_GENERIC ? 0 : occ_slot(focc)];
    }
    hipLaunchKernelGGL(fk, dim3(nblk), dim3(BLOCK), 0, st, P, sin, sin, out, c0, c1, m.sc, slot, slot_next, serial,
                       store);
    HIP_CHECK(hipGetLastError());
    dsbuf = 1 - dsbuf;
    pbuf = 1 - pbuf;
    return {nblk, BLOCK / WAVE, false};
}

DeviceSolver::StepDone DeviceSolver::step_fused_euler(const StepCtx& c) {
  Impl& m = *impl;
  if (lean_state) lean_materialize();
  // Predictor and fill of a cell run back to back in one thread, so the
  // new state goes to the other S buffer (neighbours still read the old
  // one) and the current-state index flips.
  SoA in = m.view(h, sbuf, abuf, dsbuf, pbuf);
  SoA mid = m.view(h, 1 - sbuf, abuf, 1 - dsbuf, pbuf);
  SoA out = m.view(h, 1 - sbuf, 1 - abuf, 1 - dsbuf, pbuf);
  hipLaunchKernelGGL(c.want_res ? hf2d_fused_euler<true> : hf2d_fused_euler<false>, dim3(c.nblk), dim3(BLOCK), 0,
                     m.stream, c.P, in, mid, out, c.c0, c.c1, m.sc, c.slot, c.slot_next, c.serial, m.partials);
  HIP_CHECK(hipGetLastError());
  abuf = 1 - abuf;
  dsbuf = 1 - dsbuf;
  sbuf = 1 - sbuf;
  return {c.nblk, BLOCK / WAVE, false};
}

// Lean N-S -> generic record: the split fill F_m over every cell from the
// lean state (Sp^m, level m-1 primitives), i.e. exactly the fill the split
// stepper ran (committed S, A/B/F, SrcAdd, level-m primitives, Diff and
// gradients); its dt is already in the next slot (no dt update here).
void DeviceSolver::lns_materialize() {
  p2p_complete();
  Impl& m = *impl;
  StepParams P = make_params(last_iter + iter);
  P.nx = h.nx;
  P.ny = h.ny;
  P.i0 = l_off;
  P.i1 = l_off + (gi1 - gi0);
  P.gx0 = gi0 - l_off;
  P.species = m.species;
  P.scen = m.scen;
  const Impl::Levels x = m.levels();
  if (m.mech) {
    // lean mechanism path: the split (lazy) fill F_{m+1} from Sp^{m+1}, its
    // post-kinetics species and the level-m primitives / transport; the
    // lagged k of its skip test is the state of level m
    SoA sin = m.view(h, 1 - sbuf, abuf, dsbuf, 1 - pbuf);
    m.mech_view(sin, sbuf, dsbuf);
    sin.mu = x.mu[1 - cbuf];
    sin.lam = x.lam[1 - cbuf];
    sin.mu_t = x.mu_t[1 - cbuf];
    sin.CP = x.CP[cbuf];
    sin.kk = x.kk[cbuf];
    sin.p = x.p[cbuf];
    SoA out = m.view(h, sbuf, abuf, dsbuf, pbuf);
    const long c0 = (long)P.i0 * P.ny, c1 = (long)P.i1 * P.ny;
    const unsigned nb = (unsigned)((c1 - c0 + BLOCK - 1) / BLOCK);
    // (the split fill F_{m+1} belongs to step m: its dt is slot m % 3, which
    // step m+1 has not reset yet; SST's point-implicit destruction reads it)
    hipLaunchKernelGGL((hf2d_fill_occ<SK_MECH, 9, 2, true>), dim3(nb), dim3(BLOCK), 0, m.stream, P, sin, sin, out, c0,
                       c1, m.sc, (int)((nstep + 2) % 3), -1, 0, 1);
    HIP_CHECK(hipGetLastError());
    lns_state = 0;
    cbuf = 0;
    return;
  }
  SoA sin = m.view(h, 1 - sbuf, abuf, dsbuf, 1 - pbuf);
  sin.CP = x.CP[1 - cbuf];
  sin.mu = x.mu[1 - cbuf];
  sin.lam = x.lam[1 - cbuf];
  sin.kk = x.kk[1 - cbuf];
  sin.mu_t = x.mu_t[1 - cbuf];
  SoA out = m.view(h, sbuf, abuf, dsbuf, pbuf);
  const long c0 = (long)P.i0 * P.ny, c1 = (long)P.i1 * P.ny;
  const unsigned nb = (unsigned)((c1 - c0 + BLOCK - 1) / BLOCK);
  // (the split fill F_{m+1} belongs to step m: its dt is slot m % 3, which
  // step m+1 has not reset yet; SST's point-implicit destruction reads it)
  if (sk_mode == SK_SGT)
    hipLaunchKernelGGL((hf2d_fill<SK_SGT, 1>), dim3(nb), dim3(BLOCK), 0, m.stream, P, sin, sin, out, c0, c1, m.sc,
                       (int)((nstep + 2) % 3), -1, 0, 1);
  else
    hipLaunchKernelGGL((hf2d_fill<SK_SGL, 1>), dim3(nb), dim3(BLOCK), 0, m.stream, P, sin, sin, out, c0, c1, m.sc,
                       (int)(nstep % 3), -1, 0, 1);
  HIP_CHECK(hipGetLastError());
  lns_state = 0;
  cbuf = 0;
}

// Wall heat transfer of the new state (non-adiabatic walls; the step's epilogue).
void DeviceSolver::wall_heat(const StepCtx& c) {
  Impl& m = *impl;
  hipStream_t st = m.stream;
  const StepParams& P = c.P;
  SoA s = m.view(h, sbuf, abuf, dsbuf, pbuf);
  hipLaunchKernelGGL(hf2d_wall_solid, dim3(c.nblk), dim3(BLOCK), 0, st, P, s, m.qdir, c.c0, c.c1);
  exchange(CpuSolver::HALO_QDIR);
  hipLaunchKernelGGL(hf2d_wall_wall, dim3(c.nblk), dim3(BLOCK), 0, st, P, s, m.qdir, c.c0, c.c1, m.sc, c.slot);
  HIP_CHECK(hipGetLastError());
}

void DeviceSolver::launch_chem(const StepParams& P, const SoA& mid, const SoA& out, long k0, long k1, unsigned nb,
                               int slot) {
  Impl& m = *impl;
#ifdef HF2D_FP32
  (void)P, (void)mid, (void)out, (void)k0, (void)k1, (void)nb, (void)slot, (void)m;
  throw std::runtime_error("FP32 build: finite-rate kinetics need the FP64 build");
#else
  const real* Tprev = m.Tg[pbuf];
  const MechData& md = *cs.cfg.mech->data_ptr();
  const int kind = chem_kernel ? chem_kernel : ((chem_fast && chem_fast_ok) ? 1 : (chem_rtc && chem_rtc_ok) ? 4 : 2);
  if (kind == 4) {
    if (!chem_rtc_ok) throw std::runtime_error("chem_kernel=4: hiprtc kernels unavailable: " + chem_rtc_why);
    if (chem_compact && !m.chem_list) {
      m.chem_list = m.mem.alloc<int>(h.N);
      m.chem_count = m.mem.alloc<unsigned>(1);
    }
    if (!chem_rtc_launch(md, mid, out, Tprev, k0, k1, m.sc, slot, md.Tchem, md.nsub, m.stream,
                         chem_compact ? m.chem_list : nullptr, chem_compact ? m.chem_count : nullptr))
      throw std::runtime_error("hf2d_rtc_chem launch failed");
    chem_kernel_used = "hf2d_rtc_chem";
    return;
  }
  // compiled mechanism: register-resident VALU kernel (chem_fast.hip)
  if (kind == 1) {
    if (!chem_fast_ok) throw std::runtime_error("chem_kernel=1: no compiled kernel for mechanism " + cs.cfg.mech->name);
    if (chem_compact && !m.chem_list) {
      m.chem_list = m.mem.alloc<int>(h.N);
      m.chem_count = m.mem.alloc<unsigned>(1);
    }
    if (!chem_fast_launch(cs.cfg.mech->name, P, mid, out, Tprev, k0, k1, m.sc, slot, md.Tchem, md.nsub, m.stream,
                          chem_compact ? m.chem_list : nullptr, chem_compact ? m.chem_count : nullptr))
      throw std::runtime_error("hf2d_chem_fast launch failed");
    chem_kernel_used = "hf2d_chem_fast";
    return;
  }
  // runtime mechanism: reaction-space algebra on the matrix cores (chem_mech.hip).
  // The dt of the step lives on the device: the kernel takes it from the slot.
  if (kind == 2) {
    if (!m.chem_pack) m.chem_pack = chem_mech_pack(md);
    MechCells q;
    q.S = mid.S;
    q.Yin = mid.Ys;
    q.Yout = out.Ys;
    q.Tprev = Tprev;
    q.Tout = nullptr;
    q.CT = mid.CT;
    q.N = h.N;
    q.c0 = k0;
    q.c1 = k1;
    q.Tchem = md.Tchem;
    q.dt_bits = &m.sc->dt_bits[slot];
    HIP_CHECK((hipError_t)chem_mech_launch(m.chem_pack->dev, q, 0.0, md.nsub, m.stream));
    chem_kernel_used = "hf2d_chem_mech";
    return;
  }
  chem_kernel_used = "hf2d_chem_generic";
  if (m.nsp <= 9)
    hipLaunchKernelGGL(hf2d_chem_generic<9>, dim3(nb), dim3(BLOCK), 0, m.stream, P, mid, out, Tprev, k0, k1, m.sc,
                       slot);
  else
    hipLaunchKernelGGL(hf2d_chem_generic<MECH_MAXSP>, dim3(nb), dim3(BLOCK), 0, m.stream, P, mid, out, Tprev, k0, k1,
                       m.sc, slot);
  HIP_CHECK(hipGetLastError());
#endif
}

// Called at each outer-cycle boundary by the driver (time_part restarts).
void DeviceSolver::cycle_update() {
  flush_pending();
  p2p_complete();
  Impl& m = *impl;
  if (lns_state) lns_materialize();
  if (cs.cfg.ProblemType == SM_NS && cs.cfg.semantics != Semantics::SERIAL) {
    SoA s = m.view(h, sbuf, abuf, dsbuf, pbuf);
    const int nw = (int)h.wall_own.size(), nall = (int)cs.wall_nodes.size();
    std::vector<real> v(nw);
    std::vector<uint8_t> g(nw);
    if (nw) {
      hipLaunchKernelGGL(hf2d_wall_uw, dim3((nw + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, m.stream, s, m.wall_own, nw,
                         m.wall_uw, m.wall_ok);
      HIP_CHECK(hipGetLastError());
      HIP_CHECK(hipMemcpyAsync(v.data(), m.wall_uw, nw * sizeof(real), hipMemcpyDeviceToHost, m.stream));
      HIP_CHECK(hipMemcpyAsync(g.data(), m.wall_ok, nw, hipMemcpyDeviceToHost, m.stream));
      HIP_CHECK(hipStreamSynchronize(m.stream));
    }
    std::vector<int32_t> sl;
    std::vector<real> vals;
    for (int k = 0; k < nw; k++)
      if (g[k]) {
        sl.push_back(h.wall_own_slot[k]);
        vals.push_back(v[k]);
      }
    std::vector<real> uw;
    std::vector<uint8_t> ok;
    merge_wall_uw(sl, vals, uw, ok);
    if (nall) {
      HIP_CHECK(hipMemcpyAsync(m.uw_all, uw.data(), nall * sizeof(real), hipMemcpyHostToDevice, m.stream));
      HIP_CHECK(hipMemcpyAsync(m.uw_all_ok, ok.data(), nall, hipMemcpyHostToDevice, m.stream));
      const long c0 = (long)l_off * h.ny, c1 = (long)(l_off + (gi1 - gi0)) * h.ny;
      const unsigned nb = (unsigned)((c1 - c0 + BLOCK - 1) / BLOCK);
      hipLaunchKernelGGL(hf2d_yplus, dim3(nb), dim3(BLOCK), 0, m.stream, s, c0, c1, m.uw_all, m.uw_all_ok);
      HIP_CHECK(hipGetLastError());
      // (uw and ok are pageable and end with this block: the two copies must
      // have read them before that -- a copy still queued then uploaded freed
      // memory, and with ok = 0 everywhere y+ stayed what it was)
      HIP_CHECK(hipStreamSynchronize(m.stream));
    }
  }
  HIP_CHECK(hipStreamSynchronize(m.stream));
}

// ---------------------------------------------------------------------------
// Lean single-gas N-S step (lean_ns.hpp): F_m of the tile + ring into LDS,
// predict_m from LDS, own-cell part of F_{m+1} for dt_{m+1}.  One workgroup
// per TI x TJ tile (lean_tile_geom, one cell per thread).
// ---------------------------------------------------------------------------

// FX: the multi-GPU exchange fused in (xGMI mailboxes): the cells of the
// strip's first / last two columns store this step's HALO_LNS values (Lc:
// the post-step pointers, DeviceSolver::halo_list) into the neighbour's
// mailbox, the last workgroup publishes the step and folds the peers' dt
// (fx_tail); hf2d_p2p_unpack then fills the ghost columns.
template <bool RES, int MODE, int TURB, bool FX = false>
__device__ __forceinline__ void lns_step_body(StepParams& P, const LnsArrays& a, const LeanTile& T, DevScalars* sc,
                                              int slot, int slot_next, int serial, ResidualPack* partials,
                                              int part, const FusedX& X = FusedX{}, const ColList* Lc = nullptr,
                                              const ColList* Lg = nullptr) {
  extern __shared__ real lds[];
  constexpr int NL = Lns<MODE>::NL;
  unsigned long long seq_prev = 0;
  if (FX) seq_prev = *X.seq;
  // part: 0 every tile, 1 / 2 the edge / interior tiles (comm overlap)
  // (a ghost prologue delays the strip's edge tiles: they go first, so they
  // do not finish the kernel late)
  const unsigned b = (FX && Lg != nullptr) ? tile_edge_first(xcd_remap(blockIdx.x, gridDim.x), T)
                                           : tile_of_part(xcd_remap(blockIdx.x, gridDim.x), part, T);
  apply_dt(P, sc, slot);
  if (b == 0 && threadIdx.x == 0) {
    dt_reset(sc, slot_reset(slot));
    lag_head(P, sc, slot, slot_next);
    sc->dt_bits[slot] = d_to_bits(P.dt);   // folded (later kernels of the step read the word)
    sc->time_part += P.dt;
    sc->dt_val[slot] = P.dt;
    scenario_next(P, sc, slot, slot_next);
  }
  // F_m runs with the dt of the step the split fill F_m belongs to (SST's
  // point-implicit destruction reads it); the predictor with this step's
  // (both read here: a second read of the device scalars after the fills
  // made the whole kernel 2x slower)
  const real dt_now = P.dt;
  if (MODE == SK_SGT && TURB == 3) P.dt = sc->dt_val[slot_reset(slot)];
  const int NC = T.NC;
  int i, j, c, i0, j0;
  const bool mine = lean_tile_cell(P, T, (int)b, (int)threadIdx.x, &i, &j, &c, &i0, &j0);
  int dummy = 0, skip = 0;
  // 0. the previous fused step's halo from the mailbox into the ghost columns
  if (FX && Lg != nullptr && seq_prev > 0 && !(X.skip & 4)) fx_ghost_prologue(P, X, Lg, i0, j0, T.TI, T.TJ, seq_prev);
  // 1a. ring cells first (only their S, A, B are kept)
  const int nring = 2 * (T.TI + T.TJ);
  // 1a'. a strip's first ghost column inside a partial last tile: its fill
  // is a neighbour's (the ring covers it when the tile is full).  One call
  // site for both (an inlined second copy of the fill costs registers).
#pragma unroll 1
  for (int pass = 0; pass < 2; pass++) {
    int gi = -1, gj = 0, cc = 0;
    if (pass == 0) {
      if ((int)threadIdx.x < nring) {
        int ii, jj;
        lns_ring_cell(T, (int)threadIdx.x, &ii, &jj);
        gi = i0 + ii;
        gj = j0 + jj;
        cc = (ii + 1) * T.W + jj + 1;
      }
    } else if (!mine && (int)threadIdx.x < T.TIh * T.TJ && i == P.i1 && i < P.nx && j < P.ny) {
      gi = i;
      gj = j;
      cc = c;
    }
    if (gi >= 0 && gi < P.nx && gj >= 0 && gj < P.ny) {
      CellLocal rc;
      bool early, filled;
      lns_fill_to_lds<MODE, TURB>(P, a, gi, gj, lds, NC, cc, rc, &early, &filled, &dummy);
    }
  }
  // 1b. own cell: F_m, its level-m outputs, kept values for 2./3.
  LnsLevel<MODE> lv;
  u64 CT = 0, TT = 0;
  uint8_t gf = 0, nbm = 0;
  bool early = true, filled = false;
  const long N = a.N;
  const long idx = (long)i * P.ny + j;
  real bpre[NL];
  if (mine) {
#pragma unroll
    for (int q = 0; q < NL; q++) bpre[q] = a.beta[Lns<MODE>::eqk(q) * N + idx];
    CellLocal oc;
    lns_fill_to_lds<MODE, TURB>(P, a, i, j, lds, NC, c, oc, &early, &filled, &dummy);
    CT = oc.CT;
    gf = a.gf[idx];
    nbm = a.nb[idx];
    TT = a.TT[idx];
    if (!early) {
      if (!filled) skip = 1;
      a.Uo[idx] = oc.U;
      a.Vo[idx] = oc.V;
      a.To[idx] = oc.Tg;
      a.kko[idx] = oc.k;
      a.CPo[idx] = oc.CP;
      a.lamo[idx] = oc.lam;
      a.muo[idx] = oc.mu;
      if (MODE == SK_SGT) {
        a.mu_to[idx] = oc.mu_t;
        a.Src[(long)I_K * N + idx] = oc.Src[I_K];
        a.Src[(long)I_EPS * N + idx] = oc.Src[I_EPS];
      }
      if (gf & GF_SRCADD)
#pragma unroll
        for (int q = 0; q < NL; q++) {
          const int k = Lns<MODE>::eqk(q);
          a.SrcAdd[k * N + idx] = oc.SrcAdd[k];
        }
      lv.U = oc.U;
      lv.V = oc.V;
      lv.Tg = oc.Tg;
      lv.p = oc.p;
      lv.k = oc.k;
      lv.R = oc.R;
      lv.CP = oc.CP;
      lv.lam = oc.lam;
      lv.mu = oc.mu;
      lv.mu_t = oc.mu_t;
      lv.l_min = oc.l_min;
      lv.y_plus = oc.y_plus;
      lv.BGX = oc.BGX;
      lv.BGY = oc.BGY;
#pragma unroll
      for (int q = 0; q < NL; q++) {
        const int k = Lns<MODE>::eqk(q);
        lv.SrcAdd[q] = oc.SrcAdd[k];
        lv.F[q] = oc.F[k];
        lv.Src[q] = oc.Src[k];
      }
    }
  }
  P.dt = dt_now;   // this step's dt for the predictor
  __syncthreads();
  // 2. predict_m
  ResidualPack r;
  if (RES) {
    residual_reset(r);
#pragma unroll
    for (int k = 0; k < NEQ; k++) r.eq[k].i = r.eq[k].j = -1;
  }
  double dtl = 1.0;
  int neg = 0;
  if (mine) {
    LnsPredictIO<MODE> io{a, lds, lv, bpre, N, idx, idx, idx, idx, idx, NC, c, c, c, c, c, gf, {}};
    if (!is_active(CT)) {
#pragma unroll
      for (int q = 0; q < NL; q++) {
        const int k = Lns<MODE>::eqk(q);
        io.sn[k] = io.S(k);
        io.keep_dS(k);
      }
    } else {
      const int n1 = (nbm & NB_XL) ? 1 : 0, n2 = (nbm & NB_XR) ? 1 : 0;
      const int n3 = (nbm & NB_YU) ? 1 : 0, n4 = (nbm & NB_YD) ? 1 : 0;
      io.iL = (long)(i - n1) * P.ny + j;
      io.iR = (long)(i + n2) * P.ny + j;
      io.iU = idx + n3;
      io.iD = idx - n4;
      io.cL = c - n1 * T.W;
      io.cR = c + n2 * T.W;
      io.cU = c + n3;
      io.cD = c - n4;
      predict_core<RES>(P, io, CT, TT, n1, n2, n3, n4, P.gx0 + i, j, r);
    }
#pragma unroll
    for (int q = 0; q < NL; q++) {
      const int k = Lns<MODE>::eqk(q);
      a.Sp_out[k * N + idx] = io.sn[k];
    }
    // 3. own-cell part of F_{m+1}: dt_{m+1}
    if (!early) {
      LnsOwnIO<MODE> oio(io.sn, lv, CT, TT, gf, nbm);
      CellLocal nc;
      real mY[1], mgx[1], mgy[1];
      bool e2, f2;
      dtl = fill_compute<MODE, 1, LnsOwnIO<MODE>, true>(P, oio, nc, mY, mgx, mgy, nullptr, 0, i, j, true, &neg, &e2,
                                                         &f2);
    }
  }
  if (RES) residual_publish<BLOCK>(r, partials, b);
  const double* sdt = block_dt_stage<BLOCK>(dtl);
  if (neg) atomicOr(&sc->neg_T, 1);
  if (skip) atomicOr(&sc->neg_T, LNS_SKIP_ERR);
  __syncthreads();
  if (threadIdx.x == 0) block_dt_commit<BLOCK>(sdt, sc, slot_next, serial, P.dt);
  if (FX && !(X.skip & 2)) fx_edge_push(P, X, Lc, T, i0, j0, seq_prev);
  // (unpacking the peers' halo in this last workgroup instead of a separate
  // hf2d_p2p_unpack launch measured 2x the exchange cost: one workgroup's
  // serial rounds of uncached mailbox loads, profiles/exchange_loopback_r05.md)
  if (FX && threadIdx.x < WAVE && !(X.skip & 1)) fx_tail(X, sc, slot_next, seq_prev, true, gridDim.x <= FX_COUNT1_MAX);
}

// (LnsArrays by value: passed by device pointer instead, the k-eps
// kernel spilled 215 instead of 254 SGPRs but the resonator ran 2.5 % and
// Step 3.8 % slower: the fields were re-loaded inside the fills)
template <bool RES, int MODE, int TURB = 2>
__global__ __launch_bounds__(BLOCK) void hf2d_lns_step(StepParams P, LnsArrays a, LeanTile T, DevScalars* sc,
                                                        int slot, int slot_next, int serial, ResidualPack* partials,
                                                        int part) {
  lns_step_body<RES, MODE, TURB>(P, a, T, sc, slot, slot_next, serial, partials, part);
}
// the same step with the xGMI mailbox exchange fused in (the register
// budgets of the default kernels: laminar unbounded, k-eps / SST / SA 3
// waves per SIMD)
// (FusedX and the halo column list by device pointer, as the fused tile
// kernels: SGPR spills 170 -> 252 and the resonator's 4-rank loopback
// exchange 15.8 -> 16.5 us; kept by value)
template <bool RES, int MODE, int TURB>
__global__ __launch_bounds__(BLOCK) void hf2d_lns_step_fx(StepParams P, LnsArrays a, LeanTile T, DevScalars* sc,
                                                           int slot, int slot_next, int serial,
                                                           ResidualPack* partials, FusedX X, ColList Lc,
                                                           const ColList* Lg) {
  lns_step_body<RES, MODE, TURB, true>(P, a, T, sc, slot, slot_next, serial, partials, 0, X, &Lc, Lg);
}
template <bool RES, int MODE, int TURB>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(3))) void hf2d_lns_step_fx3(
    StepParams P, LnsArrays a, LeanTile T, DevScalars* sc, int slot, int slot_next, int serial,
    ResidualPack* partials, FusedX X, ColList Lc, const ColList* Lg) {
  lns_step_body<RES, MODE, TURB, true>(P, a, T, sc, slot, slot_next, serial, partials, 0, X, &Lc, Lg);
}

// register budget of OCC waves per SIMD (DeviceSolver::lns_occ, measured)
template <bool RES, int MODE, int OCC, int TURB = 2>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(OCC))) void hf2d_lns_step_occ(
    StepParams P, LnsArrays a, LeanTile T, DevScalars* sc, int slot, int slot_next, int serial,
    ResidualPack* partials, int part) {
  lns_step_body<RES, MODE, TURB>(P, a, T, sc, slot, slot_next, serial, partials, part);
}

using LnsK = void (*)(StepParams, LnsArrays, LeanTile, DevScalars*, int, int, int, ResidualPack*, int);
// [laminar, k-eps, SST, SA][residual][register budget: default, 3, 5 waves per SIMD]
static const LnsK kLns[4][2][3] = {
    {{hf2d_lns_step<false, SK_SGL>, hf2d_lns_step_occ<false, SK_SGL, 3>, hf2d_lns_step_occ<false, SK_SGL, 5>},
     {hf2d_lns_step<true, SK_SGL>, hf2d_lns_step<true, SK_SGL>, hf2d_lns_step<true, SK_SGL>}},
    {{hf2d_lns_step<false, SK_SGT>, hf2d_lns_step_occ<false, SK_SGT, 3>, hf2d_lns_step_occ<false, SK_SGT, 5>},
     {hf2d_lns_step<true, SK_SGT>, hf2d_lns_step<true, SK_SGT>, hf2d_lns_step<true, SK_SGT>}},
    {{hf2d_lns_step<false, SK_SGT, 3>, hf2d_lns_step_occ<false, SK_SGT, 3, 3>, hf2d_lns_step_occ<false, SK_SGT, 5, 3>},
     {hf2d_lns_step<true, SK_SGT, 3>, hf2d_lns_step<true, SK_SGT, 3>, hf2d_lns_step<true, SK_SGT, 3>}},
    {{hf2d_lns_step<false, SK_SGT, 4>, hf2d_lns_step_occ<false, SK_SGT, 3, 4>, hf2d_lns_step_occ<false, SK_SGT, 5, 4>},
     {hf2d_lns_step<true, SK_SGT, 4>, hf2d_lns_step<true, SK_SGT, 4>, hf2d_lns_step<true, SK_SGT, 4>}}};

using LnsFxK = void (*)(StepParams, LnsArrays, LeanTile, DevScalars*, int, int, int, ResidualPack*, FusedX, ColList,
                        const ColList*);
// [laminar, k-eps, SST, SA][residual] (the default kernels' register budgets)
static const LnsFxK kLnsFx[4][2] = {
    {hf2d_lns_step_fx<false, SK_SGL, 2>, hf2d_lns_step_fx<true, SK_SGL, 2>},
    {hf2d_lns_step_fx3<false, SK_SGT, 2>, hf2d_lns_step_fx<true, SK_SGT, 2>},
    {hf2d_lns_step_fx3<false, SK_SGT, 3>, hf2d_lns_step_fx<true, SK_SGT, 3>},
    {hf2d_lns_step_fx3<false, SK_SGT, 4>, hf2d_lns_step_fx<true, SK_SGT, 4>}};

// The lean N-S kernel applies to this step (lean_ns.hpp; eligibility lns_ok)
bool DeviceSolver::lns_step_ok(const StepParams& P) const {
  const Impl& m = *impl;
  // (the fill F_m runs in step m here but in step m-1 in the split stepper:
  // the step parameters it reads must agree, i.e. is_mu_t must not change)
  return lean_ns && lns_ok && P.sm == SM_NS && sgl && sgl_ok && (sk_mode == SK_SGL || sk_mode == SK_SGT) &&
         !m.mech && !P.fpa.is_init && !P.ffc.is_init &&
         P.fpa.is_mu_t == lns_prev_mu_t && P.ny >= LEAN_TILE_MIN_TJ;
}

bool DeviceSolver::lns_entry(const StepParams& P0) const {
  StepParams P = P0;
  P.ny = h.ny;
  return (lean_ns && lns_ok && lns_step_ok(P)) || (lean_mech && lnm_ok && lnm_step_ok(P));
}

// Lean N-S step (lean_ns.hpp), with its entry step.
DeviceSolver::StepDone DeviceSolver::step_lean_ns(const StepCtx& c) {
  Impl& m = *impl;
  hipStream_t st = m.stream;
  const StepParams& P = c.P;
  const bool want_res = c.want_res;
  const int slot = c.slot, slot_next = c.slot_next, serial = c.serial;
  if (lean_state) lean_materialize();
  if (lns_state == 0) {
    // first lean N-S step: the split step with the fill's CP/mu/lam/k going
    // to the second level buffers (the level it read stays for K_{n+1})
    const StepDone d = step_split(c, true);
    lns_state = 1;
    cbuf = 1;
    return d;
  }
  const LnsArrays a = m.lns_arrays(h, sbuf, pbuf, cbuf, dsbuf, abuf);
  LeanTile T = lean_tile_geom(P.i1 - P.i0, P.ny, BLOCK, lean_tj > 0 ? lean_tj : lns_tile_height(P.ny, BLOCK), 1);
  // (the halo's second column must come from the edge part)
  T.ne = (P.i1 - P.i0) % T.TI == 1 ? 2 : 1;
  const int ntile = T.nbi * T.nbj;
  const bool t2 = sk_mode == SK_SGT;
  const size_t shmem = (size_t)(t2 ? Lns<SK_SGT>::PLANES : Lns<SK_SGL>::PLANES) * T.NC * sizeof(real);
  // register budget (measured, 1x MI355X): the k-eps kernel compiles to
  // ~173 VGPRs (2 waves/SIMD); a 3-wave budget is 11 % faster (resonator
  // 2000x200: 110.7 -> 98.8 us/step); the laminar one is best unbounded
  const int occ = lns_occ > 0 ? lns_occ : (t2 ? 3 : 0);
  // (a residual step runs the compiler's register budget)
  const int tv = !t2 ? 0 : lns_turb == 3 ? 2 : lns_turb == 4 ? 3 : 1;
  const LnsK lk = kLns[tv][want_res][want_res ? 0 : (occ == 5 ? 2 : occ == 3 ? 1 : 0)];
  // xGMI mailboxes: the exchange fused into the tile kernel (edge cells
  // push their HALO_LNS values to the neighbour, the last workgroup
  // publishes the step and folds the peers' dt), then one unpack kernel;
  // RCCL / in-process transports: edge tiles first, their halo on the comm
  // stream while the interior tiles compute, then the dt MIN (as the
  // inviscid tile kernel)
  const bool lns_fx = m.p2p.on && p2p_fuse && m.nranks > 1;
  const ColList Lc = lns_fx ? lns_post_list("lean N-S") : ColList{};
  // (the decision must be the same on every rank -- the exchange sequence
  // differs -- so a strip too narrow to split runs all its tiles at once)
  const bool lns_split = !lns_fx && comm_overlap && !m.p2p.on && (m.comm || m.local) && m.nranks > 1 && !want_res &&
                         cs.cfg.isAdiabaticWall;
  const bool lparts = T.nbi >= 2 + T.ne;
  if (lns_fx) {
    const ColList* Lg = claim_ghost_prologue();
    p2p_complete();   // (a list new inside a capture: the separate unpack)
    hipLaunchKernelGGL(kLnsFx[tv][want_res ? 1 : 0], dim3(ntile), dim3(BLOCK), shmem, st, P, a, T, m.sc, slot,
                       slot_next, serial, m.partials, fused_args(), Lc, Lg);
    HIP_CHECK(hipGetLastError());
    m.lns_pend = Lc;
    lns_ghost_pending = lns_last_valid = true;   // unpacked by the next fused step or p2p_complete
    if (lns_ghost_prologue) (void)lc_device(Lc);   // (uploaded now, outside any capture, when eager)
    ghost_stale = true;   // lean representation in the ghosts
    lns_fx_steps++;
  } else if (lns_split) {
    overlap_streams();
    hipLaunchKernelGGL(lk, dim3(lparts ? (1 + T.ne) * T.nbj : ntile), dim3(BLOCK), shmem, st, P, a, T, m.sc, slot,
                       slot_next, serial, m.partials, lparts ? 1 : 0);
  } else {
    hipLaunchKernelGGL(lk, dim3(ntile), dim3(BLOCK), shmem, st, P, a, T, m.sc, slot, slot_next, serial,
                       m.partials, 0);
  }
  HIP_CHECK(hipGetLastError());
  flip_state();
  cbuf = 1 - cbuf;
  lns_steps++;
  if (lns_split) {
    HIP_CHECK(hipEventRecord(m.ev_edge, st));
    // interior tiles in flight before the exchange is issued; they write
    // neither the edge columns nor the ghost columns
    if (lparts)
      hipLaunchKernelGGL(lk, dim3((T.nbi - 1 - T.ne) * T.nbj), dim3(BLOCK), shmem, st, P, a, T, m.sc, slot,
                         slot_next, serial, m.partials, 2);
    HIP_CHECK(hipGetLastError());
    overlap_exchange(CpuSolver::HALO_LNS, slot_next);
  }
  // (fused: exchanged inside the kernel, unpacked by the next step or p2p_complete)
  return {(unsigned)ntile, BLOCK / WAVE, lns_fx || lns_split};
}

// ---------------------------------------------------------------------------
// Lean mechanism-mode step (lean_mech.hpp): hf2d_lnm_step per 16 x 16 tile,
// then the kinetics of the listed cells and hf2d_lnm_hot.
// ---------------------------------------------------------------------------
// G_m of global cell (gi, gj) at tile coordinates (ii, jj): flow S / A / B
// and species A / B into the LDS planes that cell feeds.  dt_fill: the dt of
// the step the split fill F_m belongs to (SST's point-implicit destruction).
template <int TURB>
__device__ __forceinline__ void lnm_fill(StepParams& P, const LnmArrays& a, const LnmLayout& L, real* lds, int gi,
                                         int gj, int ii, int jj, CellLocal& c, real* mY, bool* early, bool* filled) {
  LnmFillIO<TURB> io(a, gi, gj, P.nx, P.ny);
  io.lds = lds;
  io.L = &L;
  io.aoff = L.a_at(ii, jj);
  io.boff = L.b_at(ii, jj);
  real mgx[1], mgy[1];
  int dummy = 0;
  (void)fill_compute<SK_MECH, LNM_NSB, LnmFillIO<TURB>, true>(P, io, c, mY, mgx, mgy, a.mech, a.nsp, gi, gj, true,
                                                               &dummy, early, filled);
  const int sC = L.s_at(ii, jj), aC = io.aoff, bC = io.boff;
  const bool zero = *early || !*filled;
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const int k = Lns<SK_SGT>::eqk(q);
    lds[L.oS + q * L.NC + sC] = c.S[k];
    if (aC >= 0) lds[L.oA + q * L.NA + aC] = zero ? 0.0 : c.A[k];
    if (bC >= 0) lds[L.oB + q * L.NB + bC] = zero ? 0.0 : c.B[k];
  }
  if (zero)   // (a skipped node stops the lean path; a solid one is never a neighbour)
    for (int t = 0; t < L.nspt; t++) {
      if (aC >= 0) lds[L.osA + t * L.NA + aC] = 0.0;
      if (bC >= 0) lds[L.osB + t * L.NB + bC] = 0.0;
    }
}

// STRIP: the strip has a right neighbour, so a partial last tile may hold its
// first ghost column (pass 1 below); without it the fill runs in one pass
// (56 instead of 112 B/lane of scratch for the SST kernel)
template <bool RES, int TURB, bool STRIP = true>
__device__ __forceinline__ void lnm_step_body(StepParams& P, const LnmArrays& a, const LeanTile& T, DevScalars* sc,
                                              int slot, int slot_next, int serial, ResidualPack* partials) {
  extern __shared__ real lds[];
  const unsigned b = a.lg ? tile_edge_first(xcd_remap(blockIdx.x, gridDim.x), T)
                          : tile_of_part(xcd_remap(blockIdx.x, gridDim.x), a.part, T);
  const LnmLayout L(T.TI, T.TJ, a.nsp - 1);
  // phase trace: wavefront 0 (slots 0..8) and the last wavefront (9, 10) of the workgroup
  unsigned long long* tr = a.tr ? a.tr + (long)b * 12 : nullptr;
  const bool tr0 = tr && threadIdx.x == 0, trl = tr && threadIdx.x == BLOCK - WAVE;
  if (tr0) tr[0] = rt_clock();
  // G_m runs with the dt of the step the split fill F_m belongs to; this
  // step's dt, scenario values and dt/dx, dt/dy are read up front as well (a
  // second read of the device scalars after the fills doubled the lean N-S
  // kernel's time)
  apply_dt(P, sc, slot);
  const real dt_now = P.dt;
  P.dt = sc->dt_val[slot_reset(slot)];
  const real dt_step = dt_cur(P, sc, slot);
  if (b == 0 && threadIdx.x == 0) {
    dt_reset(sc, slot_reset(slot));
    lag_head(P, sc, slot, slot_next);
    sc->dt_bits[slot] = d_to_bits(dt_step);   // folded (the kinetics read the word)
    sc->time_part += dt_step;
    sc->dt_val[slot] = dt_step;
    sc->hot_cnt[slot_next] = 0;
    // the interior tiles' list of a comm-overlap step (a later launch of this
    // step) starts empty whatever ran before (split steps reset hot_cnt only)
    sc->hot_cnt2[slot] = 0;
    scenario_next(P, sc, slot, slot_next);
  }
  int i, j, c, i0, j0;
  const bool mine = lean_tile_cell(P, T, (int)b, (int)threadIdx.x, &i, &j, &c, &i0, &j0);
  const int ii = (int)threadIdx.x / T.TJ, jj = (int)threadIdx.x - ii * T.TJ;
  int skip = 0;
  // 0. the previous step's halo from the mailbox into the ghost columns
  if (a.lg) {
    const FusedX& X = *a.xg;
    const unsigned long long seq_prev = *X.seq;
    if (seq_prev > 0 && !(X.skip & 4)) fx_ghost_prologue(P, X, a.lg, i0, j0, T.TI, T.TJ, seq_prev);
  }
  // 1a. ring cells: S, A or B only (on the threads after the tile's cells when
  // they fit in the workgroup, else on the first ones as a second fill)
  const int nring = 2 * (T.TI + T.TJ), own = T.TI * T.TJ;
  const int rbase = own + nring <= BLOCK ? own : 0;
  const int rt = (int)threadIdx.x - rbase;
  // 1a'. a strip's first ghost column inside a partial last tile (see lns).
  // Both fills go through one call site: a second inlined copy of the fill
  // pushed the SST kernel from 56 to 784 B/lane of scratch (2x slower).
#pragma unroll 1
  for (int pass = 0; pass < (STRIP ? 2 : 1); pass++) {
    int gi = -1, gj = 0, ri = 0, rj = 0;
    if (pass == 0) {
      if (rt >= 0 && rt < nring) {
        lns_ring_cell(T, rt, &ri, &rj);
        gi = i0 + ri;
        gj = j0 + rj;
      }
    } else if (!mine && (int)threadIdx.x < T.TIh * T.TJ && i == P.i1 && i < P.nx && j < P.ny) {
      gi = i;
      gj = j;
      ri = ii;
      rj = jj;
    }
    if (gi >= 0 && gi < P.nx && gj >= 0 && gj < P.ny) {
      CellLocal rc;
      real mY[LNM_NSB];
      bool early, filled;
      lnm_fill<TURB>(P, a, L, lds, gi, gj, ri, rj, rc, mY, &early, &filled);
    }
    if (pass == 0 && tr0) tr[1] = rt_clock();
  }
  // 1b. own cell: G_m, its level-m outputs, kept values for 2. and 3.
  LnmLevel lv;
  u64 CT = 0;
  uint8_t gf = 0, nbm = 0;
  bool early = true;
  const long N = a.N;
  const long idx = (long)i * P.ny + j;
  real bpre[6];
  if (mine) {
#pragma unroll
    for (int q = 0; q < 6; q++) bpre[q] = a.beta[Lns<SK_SGT>::eqk(q) * N + idx];
    CellLocal oc;
    real mY[LNM_NSB];
    bool filled = false;
    lnm_fill<TURB>(P, a, L, lds, i, j, ii, jj, oc, mY, &early, &filled);
    CT = oc.CT;
    gf = a.gf[idx];
    nbm = a.nb[idx];
    if (!early) {
      if (!filled) skip = 1;
      // mixture transport at T^m (fill_compute's tail: active nodes with a valid T)
      real mu = oc.mu, lam = oc.lam;
      if (is_active(CT) && !(oc.Tg < 0. || !(oc.Tg > MECH_TMIN))) mech_transport<LNM_NSB>(*a.mech, mY, oc.Tg, &mu, &lam);
      a.Uo[idx] = oc.U;
      a.Vo[idx] = oc.V;
      a.To[idx] = oc.Tg;
      a.muo[idx] = mu;
      a.lamo[idx] = lam;
      a.mu_to[idx] = oc.mu_t;
      if (TURB) {
        a.Src[(long)I_K * N + idx] = oc.Src[I_K];
        a.Src[(long)I_EPS * N + idx] = oc.Src[I_EPS];
      }
      if (gf & GF_SRCADD)
#pragma unroll
        for (int q = 0; q < 6; q++) {
          const int k = Lns<SK_SGT>::eqk(q);
          a.SrcAdd[k * N + idx] = oc.SrcAdd[k];
        }
      lv.U = oc.U;
      lv.V = oc.V;
      lv.Tg = oc.Tg;
      lv.k = oc.k;
      lv.BGX = oc.BGX;
      lv.BGY = oc.BGY;
#pragma unroll
      for (int q = 0; q < 6; q++) {
        const int k = Lns<SK_SGT>::eqk(q);
        lv.SrcAdd[q] = oc.SrcAdd[k];
        lv.F[q] = oc.F[k];
        lv.Src[q] = oc.Src[k];
      }
    }
  }
  if (tr0) tr[2] = rt_clock();
  if (trl) tr[9] = rt_clock();
  // species inputs of the predictor, loaded before the barrier (in flight
  // while the other wavefronts finish their fills)
  const int n1 = (nbm & NB_XL) ? 1 : 0, n2 = (nbm & NB_XR) ? 1 : 0;
  const int n3 = (nbm & NB_YU) ? 1 : 0, n4 = (nbm & NB_YD) ? 1 : 0;
  const long iL = (long)(i - n1) * P.ny + j, iR = (long)(i + n2) * P.ny + j, iU = idx + n3, iD = idx - n4;
  real ys0[LNM_NSB], ysL[LNM_NSB], ysR[LNM_NSB], ysU[LNM_NSB], ysD[LNM_NSB], bts[LNM_NSB];
  if (mine) {
#pragma unroll
    for (int s = 0; s < LNM_NSB; s++) {
      const long o = (long)(s < a.nsp ? s : a.nsp - 1) * N;
      ys0[s] = a.Ys[o + idx];
      ysL[s] = a.Ys[o + iL];
      ysR[s] = a.Ys[o + iR];
      ysU[s] = a.Ys[o + iU];
      ysD[s] = a.Ys[o + iD];
      bts[s] = a.betas[o + idx];
    }
  }
  P.dt = dt_now;   // this step's dt for the predictor and E_{m+1}
  __syncthreads();
  if (tr0) tr[3] = rt_clock();
  // 2. predict_m, flow and turbulence equations
  ResidualPack r;
  if (RES) {
    residual_reset(r);
#pragma unroll
    for (int k = 0; k < NEQ; k++) r.eq[k].i = r.eq[k].j = -1;
  }
  real dtl = 1.0;
  int neg = 0;
  const int nsp = a.nsp, bath = a.bath;
  if (mine) {
    const int sC = L.s_at(ii, jj), aC = L.a_at(ii, jj), bC = L.b_at(ii, jj);
    LnmPredictIO io{a, lds, L, lv, bpre, N, idx, idx, idx, idx, idx, sC, sC, sC, sC, sC, aC, aC, bC, bC, gf, {}};
    const bool act = is_active(CT);
    const u64 TT = a.TT[idx];
    if (!act) {
#pragma unroll
      for (int q = 0; q < 6; q++) {
        const int k = Lns<SK_SGT>::eqk(q);
        io.sn[k] = io.S(k);
        io.keep_dS(k);
      }
    } else {
      io.iL = iL;
      io.iR = iR;
      io.iU = iU;
      io.iD = iD;
      io.sL = sC - n1 * (T.TJ + 2);
      io.sR = sC + n2 * (T.TJ + 2);
      io.sU = sC + n3;
      io.sD = sC - n4;
      io.aL = aC - n1 * T.TJ;
      io.aR = aC + n2 * T.TJ;
      io.bU = bC + n3;
      io.bD = bC - n4;
      predict_core<RES>(P, io, CT, TT, n1, n2, n3, n4, P.gx0 + i, j, r);
    }
#pragma unroll
    for (int q = 0; q < 6; q++) {
      const int k = Lns<SK_SGT>::eqk(q);
      a.Sp_out[k * N + idx] = io.sn[k];
    }
    if (tr0) tr[4] = rt_clock();
    // 3. species: transported ones by the predictor, the bath gas as the
    // remainder of the new rho (predict_cell_t order)
    real ysn[LNM_NSB];
    real sum = 0.0;
    const real rho_c = io.S(I_RHO);
#pragma unroll
    for (int s = 0; s < LNM_NSB; s++) {
      ysn[s] = 0.0;
      if (s < nsp && (s != bath || !act)) {
        const long o = (long)s * N;
        LnmSpeciesIO sio{a, lds, L, N, idx, iL, iR, iU, iD, o, s < bath ? s : s - 1, io.aL, io.aR, io.bU, io.bD, bC,
                         gf, ys0[s], ysL[s], ysR[s], ysU[s], ysD[s], bts[s], lv.SrcAdd[0], rho_c, 0.0};
        if (!act) {
          sio.out = sio.ys;
          a.Ys_out[o + idx] = sio.ys;
          sio.keep_dS(0);
        } else {
          predict_core<RES>(P, sio, CT, TT, n1, n2, n3, n4, P.gx0 + i, j, r);
          sum += sio.out;
        }
        ysn[s] = sio.out;
      }
    }
    if (act)
#pragma unroll
      for (int s = 0; s < LNM_NSB; s++)
        if (s == bath) {
          ysn[s] = io.sn[I_RHO] - sum;
          a.Ys_out[(long)s * N + idx] = ysn[s];
        }
    if (tr0) tr[5] = rt_clock();
    // 4. E_{m+1} of the new state, unless the kinetics change it (then hf2d_lnm_hot)
    if (!early) {
      const bool hot = act && io.sn[I_RHO] > 0.0 && lv.Tg >= a.mech->Tchem && P.dt > 0.0;
      const unsigned long long ball = __ballot(hot);
      if (ball) {
        const int lane = threadIdx.x & (WAVE - 1);
        const int leader = __ffsll((long long)ball) - 1;
        unsigned base = 0;
        if (lane == leader) base = atomicAdd(a.hot_n, (unsigned)__popcll(ball));
        base = __shfl(base, leader, WAVE);
        if (hot) a.hot[base + __popcll(ball & ((1ull << lane) - 1ull))] = (int)idx;
      }
      if (!hot) {
        const real S4[4] = {io.sn[0], io.sn[1], io.sn[2], io.sn[3]};
        LnmState st;
        if (!mech_state_node(P, *a.mech, nsp, S4, ysn, lv.U, lv.V, lv.Tg, lv.k, CT, lv.BGX, lv.BGY, &st, &dtl, &neg))
          skip = 1;
        a.Tso[idx] = st.T;
        a.pso[idx] = st.p;
        a.CPso[idx] = st.CP;
        a.kso[idx] = st.k;
      }
    }
  }
  if (tr0) tr[6] = rt_clock();
  if (trl) tr[10] = rt_clock();
  // (residual_publish and the dt reduction written out: profiles/step_epilogue_ab.md)
  if (RES) {
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) shfl_merge(r, off);
    if ((threadIdx.x & (WAVE - 1)) == 0) partials[(long)b * (BLOCK / WAVE) + threadIdx.x / WAVE] = r;
  }
  for (int off = 1; off < WAVE; off <<= 1) dtl = fmin(dtl, __shfl_xor(dtl, off, WAVE));
  __shared__ double sdt[BLOCK / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) sdt[threadIdx.x / WAVE] = dtl;
  if (neg) atomicOr(&sc->neg_T, 1);
  if (skip) atomicOr(&sc->neg_T, LNS_SKIP_ERR);
  __syncthreads();
  if (threadIdx.x == 0) {
    double mn = sdt[0];
    for (int q = 1; q < BLOCK / WAVE; q++) mn = fmin(mn, sdt[q]);
    if (serial) mn = fmin(mn, P.dt);
    dt_min(sc, slot_next, mn);
  }
  if (tr0) {
    tr[7] = rt_clock();
    tr[8] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID: wave/SIMD/CU/SE
    tr[11] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
  }
}

// (two workgroups per CU: the LDS of a 16 x 16 tile is ~80 KB, so a budget
// of 2 waves per SIMD costs no occupancy)
template <bool RES, int TURB, bool STRIP = true>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2))) void hf2d_lnm_step(
    StepParams P, LnmArrays a, LeanTile T, DevScalars* sc, int slot, int slot_next, int serial,
    ResidualPack* partials) {
  lnm_step_body<RES, TURB, STRIP>(P, a, T, sc, slot, slot_next, serial, partials);
}

// E_{m+1} of the cells the kinetics changed (after them): state and dt.
__global__ __launch_bounds__(BLOCK) void hf2d_lnm_hot(StepParams P, LnmArrays a, DevScalars* sc, int slot,
                                                       int slot_next, int serial) {
  apply_dt(P, sc, slot);
  const unsigned n = *a.hot_n;
  const long N = a.N;
  real dtl = 1.0;
  int neg = 0, skip = 0;
  for (unsigned q = blockIdx.x * BLOCK + threadIdx.x; q < n; q += gridDim.x * BLOCK) {
    const long idx = a.hot[q];
    real S4[4], ys[LNM_NSB];
#pragma unroll
    for (int k = 0; k < 4; k++) S4[k] = a.Sp_out[k * N + idx];
#pragma unroll
    for (int s = 0; s < LNM_NSB; s++) ys[s] = a.Ys_out[(long)(s < a.nsp ? s : a.nsp - 1) * N + idx];
    LnmState st;
    real d = 1.0;
    if (!mech_state_node(P, *a.mech, a.nsp, S4, ys, a.Uo[idx], a.Vo[idx], a.To[idx], a.ksi[idx], a.CT[idx],
                         a.BGX[idx], a.BGY[idx], &st, &d, &neg))
      skip = 1;
    dtl = fmin(dtl, d);
    a.Tso[idx] = st.T;
    a.pso[idx] = st.p;
    a.CPso[idx] = st.CP;
    a.kso[idx] = st.k;
  }
  const double* sdt = block_dt_stage<BLOCK>(dtl);
  if (neg) atomicOr(&sc->neg_T, 1);
  if (skip) atomicOr(&sc->neg_T, LNS_SKIP_ERR);
  __syncthreads();
  // (a workgroup without a listed cell sends nothing)
  if (threadIdx.x == 0) block_dt_commit<BLOCK>(sdt, sc, slot_next, serial, P.dt, DT_HAVE_SLOT, DT_SKIP_UNSET);
}

// The lean mechanism step applies (lean_mech.hpp; eligibility lnm_ok) with a
// list-building kinetics kernel (compiled or hiprtc-specialised)
bool DeviceSolver::lnm_step_ok(const StepParams& P) const {
  const Impl& m = *impl;
  const int kind = chem_kernel ? chem_kernel : ((chem_fast && chem_fast_ok) ? 1 : (chem_rtc && chem_rtc_ok) ? 4 : 2);
  return lean_mech && lnm_ok && m.mech && P.sm == SM_NS && chem_compact &&
         ((kind == 1 && chem_fast_ok) || (kind == 4 && chem_rtc_ok)) && !P.fpa.is_init && !P.ffc.is_init &&
         P.fpa.is_mu_t == lns_prev_mu_t && P.ny >= LNM_TILE;
}

using LnmK = void (*)(StepParams, LnmArrays, LeanTile, DevScalars*, int, int, int, ResidualPack*);
// [residual][SST]
// [residual][SST][strip with a right neighbour] (residual steps: the strip variant)
static const LnmK kLnm[2][2][2] = {
    {{hf2d_lnm_step<false, 0, false>, hf2d_lnm_step<false, 0, true>},
     {hf2d_lnm_step<false, 3, false>, hf2d_lnm_step<false, 3, true>}},
    {{hf2d_lnm_step<true, 0>, hf2d_lnm_step<true, 0>}, {hf2d_lnm_step<true, 3>, hf2d_lnm_step<true, 3>}}};

std::vector<unsigned long long> DeviceSolver::lnm_trace_fetch() {
  synchronize();
  Impl& m = *impl;
  std::vector<unsigned long long> v((size_t)m.lnm_trace_n * 12);
  if (!v.empty()) HIP_CHECK(hipMemcpy(v.data(), m.lnm_trace, v.size() * 8, hipMemcpyDeviceToHost));
  return v;
}

// One lean mechanism step (lean_mech.hpp): tile kernel, kinetics of the
// listed cells in place on the new species, their state kernel.
DeviceSolver::StepDone DeviceSolver::lnm_step(const StepCtx& c) {
  Impl& m = *impl;
  hipStream_t st = m.stream;
  const StepParams& P = c.P;
  const bool want_res = c.want_res;
  const int slot = c.slot, slot_next = c.slot_next, serial = c.serial;
  if (lean_state) lean_materialize();
  if (lns_state == 0) {
    // first lean mechanism step: the split step, then T^{n+1} as the stored state.
    // Its fill F_{n+1} overwrites the level-n state (Cp, k, p) in place; a
    // materialise right after this step (a download after a one-step call)
    // re-runs F_{n+1}, which reads the lagged state from the [cbuf] buffers
    // as after a lean step: keep level n there (without it the re-fill read
    // stale buffers: with a download after every step the scramjet's dt
    // left the CPU stepper's at step 4; test_download_after_every_step_leaves_the_trajectory_unchanged)
    const size_t SB = (size_t)h.N * sizeof(real);
    HIP_CHECK(hipMemcpyAsync(m.CP2, m.CP, SB, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.kk2, m.kk, SB, hipMemcpyDeviceToDevice, st));
    HIP_CHECK(hipMemcpyAsync(m.p2, m.p, SB, hipMemcpyDeviceToDevice, st));
    const StepDone d = step_split(c, true);
    HIP_CHECK(hipMemcpyAsync(m.Tst[0], m.Tg[pbuf], h.N * sizeof(real), hipMemcpyDeviceToDevice, st));
    lns_state = 1;
    cbuf = 1;
    return d;
  }
  LnmArrays a = m.lnm_arrays(h, sbuf, pbuf, cbuf, dsbuf, abuf);
  if (lnm_trace) {   // phase trace of every step (the last one is kept)
    const long nwg = (long)((P.i1 - P.i0 + lnm_ti - 1) / lnm_ti) * ((P.ny + LNM_TILE - 1) / LNM_TILE);
    if (!m.lnm_trace || m.lnm_trace_n < nwg) {
      m.lnm_trace = m.mem.alloc<unsigned long long>(nwg * 12);
      m.lnm_trace_n = nwg;
    }
    a.tr = m.lnm_trace;
  }
  if (lnm_ti < 1 || lnm_ti > BLOCK / LNM_TILE) lnm_ti = BLOCK / LNM_TILE;
  LeanTile T = lnm_tile(P.i1 - P.i0, P.ny, lnm_ti);
  T.ne = (P.i1 - P.i0) % T.TI == 1 ? 2 : 1;   // (the halo's second column from the edge part)
  // RCCL / in-process transports: the tiles of the strip's first and last
  // tile columns first -- with their kinetics and state kernel, which change
  // the reacting edge cells' halo values -- then their halo on the comm
  // stream while the interior tiles and their kinetics run (a second list),
  // then the dt MIN (as the lean N-S and inviscid tile kernels)
  // (the decision must be the same on every rank -- the exchange sequence
  // differs -- so a strip too narrow to split runs all its tiles at once)
  // Opt-in (lnm_overlap): the edge part is one
  // workgroup round of ~50 tiles on an otherwise idle GPU before the interior
  // starts, so on the mailbox transport the split step measured 109 us of
  // exchange cost against 17 us for all tiles + push / unpack
  // (tools/exchange_loopback.py, scramjet 8 ranks, profiles/exchange_loopback_r05.md)
  const bool lnm_split = lnm_overlap && comm_overlap &&
                         (m.p2p.on ? p2p_fuse : (m.comm || m.local)) && m.nranks > 1 && !want_res &&
                         cs.cfg.isAdiabaticWall;
  const bool parts = T.nbi >= 2 + T.ne;
  // (xGMI mailboxes: the edge halo is pushed before the interior tiles run,
  // and published with the dt once they are done)
  const ColList Lc = lnm_split && m.p2p.on ? lns_post_list("mechanism") : ColList{};
  if (!lnm_split) {
    a.hot = m.chem_list;
    a.hot_n = &m.sc->hot_cnt[slot];
    a.part = 0;
    // mailboxes: the previous step's halo (pushed after its state kernel,
    // exchange()) is unpacked by this step's edge tiles (fx_ghost_prologue)
    if (m.p2p.on && p2p_fuse && m.nranks > 1) a.lg = claim_ghost_prologue();
    if (a.lg) a.xg = fx_device(fused_args());
    p2p_complete();
    lnm_launch(P, a, T, want_res, slot, slot_next, serial, (unsigned)(T.nbi * T.nbj));
  } else {
    p2p_complete();
    overlap_streams();
    // edge list first (at most its own cells), the interior list after it:
    // tile column 0 (TI columns), ne - 1 full columns and the last, partial
    // one of w - (nbi - 1) TI columns -- the list holds exactly N entries
    const long wl = (long)(P.i1 - P.i0) - (long)(T.nbi - 1) * T.TI;
    const long edge_cells = ((long)T.ne * T.TI + wl) * P.ny;
    a.hot = m.chem_list;
    a.hot_n = &m.sc->hot_cnt[slot];
    a.part = parts ? 1 : 0;
    lnm_launch(P, a, T, want_res, slot, slot_next, serial, (unsigned)(parts ? (1 + T.ne) * T.nbj : T.nbi * T.nbj));
    if (m.p2p.on) {
      p2p_push(Lc, st, slot_next, 1, 0);
    } else {
      HIP_CHECK(hipEventRecord(m.ev_edge, st));
    }
    a.hot = m.chem_list + edge_cells;
    a.hot_n = &m.sc->hot_cnt2[slot];
    a.part = 2;
    if (parts) lnm_launch(P, a, T, want_res, slot, slot_next, serial, (unsigned)((T.nbi - 1 - T.ne) * T.nbj));
    if (m.p2p.on) {
      p2p_finish(slot_next);
      p2p_unpack(Lc, st);
      ghost_stale = true;
      p2p_mwg_exchanges++;
      overlap_steps++;
    }
  }
  flip_state();
  cbuf = 1 - cbuf;
  lnm_steps++;
  // the new state's halo (post-step buffers), overlapped with the interior
  if (lnm_split && !m.p2p.on) overlap_exchange(CpuSolver::HALO_LNS, slot_next);
  return {(unsigned)(T.nbi * T.nbj), BLOCK / WAVE, lnm_split};
}

// Tile kernel (the tiles of a.part), kinetics of the cells it listed (a.hot /
// a.hot_n) in place on the new species, their state kernel.
void DeviceSolver::lnm_launch(const StepParams& P, const LnmArrays& a, const LeanTile& T, bool want_res, int slot,
                              int slot_next, int serial, unsigned ntile) {
  Impl& m = *impl;
  hipStream_t st = m.stream;
  const LnmLayout L(T.TI, T.TJ, m.nsp - 1);
  const size_t shmem = (size_t)L.total() * sizeof(real);
  const int strip = P.i1 < P.nx ? 1 : 0;
  const LnmK k = kLnm[want_res ? 1 : 0][lnm_turb == 3 ? 1 : 0][strip];
  // the dynamic-LDS limit is a property of the kernel function, shared by
  // every solver of the process (virtual ranks run on threads): raise it to
  // the largest layout asked for so far (tile width / species count vary)
  static std::atomic<int> attr_bytes[2][2][2] = {};
  static std::mutex attr_mu;
  std::atomic<int>& ab = attr_bytes[want_res ? 1 : 0][lnm_turb == 3 ? 1 : 0][strip];
  if (ab.load(std::memory_order_acquire) < (int)shmem) {
    std::lock_guard<std::mutex> lk(attr_mu);
    if (ab.load(std::memory_order_relaxed) < (int)shmem) {
      HIP_CHECK(hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
      ab.store((int)shmem, std::memory_order_release);
    }
  }
  // lnm_timing: events around the three phases (measurement only: the host
  // waits for each step's events, so the steps serialise with the host)
  if (lnm_timing) {
    if (!m.lnm_ev[0])
      for (auto& e : m.lnm_ev) HIP_CHECK(hipEventCreate(&e));
    HIP_CHECK(hipEventRecord(m.lnm_ev[0], st));
  }
  hipLaunchKernelGGL(k, dim3(ntile), dim3(BLOCK), shmem, st, P, a, T, m.sc, slot, slot_next, serial, m.partials);
  HIP_CHECK(hipGetLastError());
  if (lnm_timing) HIP_CHECK(hipEventRecord(m.lnm_ev[1], st));
  // kinetics of the listed cells (T^m >= Tchem), in place on the new species
  const MechData& md = *cs.cfg.mech->data_ptr();
  SoA mid;
  mid.nx = h.nx;
  mid.ny = h.ny;
  mid.N = h.N;
  mid.S = a.Sp_out;
  mid.Ys = a.Ys_out;
  mid.CT = m.CT;
  mid.mech = m.mech;
  mid.nsp = m.nsp;
  const long c0 = (long)P.i0 * P.ny, c1 = (long)P.i1 * P.ny;
  const int kind = chem_kernel ? chem_kernel : ((chem_fast && chem_fast_ok) ? 1 : 4);
#ifdef HF2D_FP32
  (void)kind, (void)c0, (void)c1, (void)md;
  throw std::runtime_error("FP32 build: finite-rate kinetics need the FP64 build");
#else
  if (kind == 1) {
    if (!chem_fast_launch(cs.cfg.mech->name, P, mid, mid, a.To, c0, c1, m.sc, slot, md.Tchem, md.nsub, st, a.hot,
                          a.hot_n, true))
      throw std::runtime_error("hf2d_chem_fast list launch failed");
    chem_kernel_used = "hf2d_chem_fast";
  } else {
    if (!chem_rtc_launch(md, mid, mid, a.To, c0, c1, m.sc, slot, md.Tchem, md.nsub, st, a.hot, a.hot_n, true))
      throw std::runtime_error("hf2d_rtc_chem list launch failed");
    chem_kernel_used = "hf2d_rtc_chem";
  }
#endif
  if (lnm_timing) HIP_CHECK(hipEventRecord(m.lnm_ev[2], st));
  const unsigned nb = (unsigned)std::min<long>((c1 - c0 + BLOCK - 1) / BLOCK, 1024);
  hipLaunchKernelGGL(hf2d_lnm_hot, dim3(nb), dim3(BLOCK), 0, st, P, a, m.sc, slot, slot_next, serial);
  HIP_CHECK(hipGetLastError());
  if (lnm_timing) {
    HIP_CHECK(hipEventRecord(m.lnm_ev[3], st));
    HIP_CHECK(hipEventSynchronize(m.lnm_ev[3]));
    for (int q = 0; q < 3; q++) {
      float ms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&ms, m.lnm_ev[q], m.lnm_ev[q + 1]));
      lnm_phase_ms[q] += ms;
    }
    lnm_phase_ms[3] += 1.0;
  }
}

}  // namespace hf2d
