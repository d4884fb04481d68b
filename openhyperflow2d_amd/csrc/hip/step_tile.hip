// Inviscid lean steps: the LDS-tiled kernels (lean_tile.hpp), the flat lean
// Euler kernel of the first lean step, the lean -> generic materialize, their
// tables and the DeviceSolver members that launch them.

#include "device_impl.hpp"
#include "lean_tile.hpp"

namespace hf2d {

template <bool RES, bool FROMG>
__global__ __launch_bounds__(BLOCK) void hf2d_lean_euler(StepParams P, LeanSoA L, long c0, long c1, DevScalars* sc,
                                                          int slot, int slot_next, int serial,
                                                          ResidualPack* partials) {
  apply_dt(P, sc, slot);
  const unsigned b = xcd_remap(blockIdx.x, gridDim.x);
  const long g = (long)b * BLOCK + threadIdx.x;
  if (g == 0) step_head(P, sc, slot, slot_next, P.dt);
  const long c = c0 + g;
  ResidualPack r;
  if (RES) residual_begin(r);
  double dtl = 1.0;
  int neg = 0;
  if (c < c1) {
    const auto [i, j] = cell_ij(c, P.ny);
    dtl = lean_euler_cell<RES, FROMG>(P, L, i, j, r, &neg);
  }
  if (RES) residual_publish<BLOCK>(r, partials, b);
  const double* sdt = block_dt_stage<BLOCK>(dtl);
  if (neg) atomicOr(&sc->neg_T, 1);
  __syncthreads();
  if (threadIdx.x == 0) block_dt_commit<BLOCK>(sdt, sc, slot_next, serial, P.dt);
}

__global__ __launch_bounds__(BLOCK) void hf2d_lean_materialize(StepParams P, LeanSoA L, SoA g, long c0, long c1) {
  const long c = c0 + (long)blockIdx.x * BLOCK + threadIdx.x;
  if (c >= c1) return;
  const auto [i, j] = cell_ij(c, P.ny);
  lean_materialize_cell(P, L, g, i, j);
}

// ---------------------------------------------------------------------------
// Kernel tables: the template variants a step can select, indexed by the
// selecting parameters (the host dispatch is a table lookup, not a ladder).
// ---------------------------------------------------------------------------

using TileK = void (*)(StepParams, LeanSoA, LeanTile, DevScalars*, int, int, int, ResidualPack*, int);
using TileFxK = void (*)(StepParams, LeanSoA, LeanTile, DevScalars*, int, int, int, ResidualPack*, const FusedX*);
using TileTrK = void (*)(StepParams, LeanSoA, LeanTile, DevScalars*, int, int, int, ResidualPack*,
                         unsigned long long*);
// [single gas][cells per thread - 1][0 plain, 1 outputs, 2 residual]
static const TileK kTile[2][2][3] = {
    {{hf2d_lean_tile<false, false, false, 0, 1>, hf2d_lean_tile<false, true, false, 0, 1>,
      hf2d_lean_tile<true, true, false, 0, 1>},
     {hf2d_lean_tile<false, false, false, 0, 2>, hf2d_lean_tile<false, true, false, 0, 2>,
      hf2d_lean_tile<true, true, false, 0, 2>}},
    {{hf2d_lean_tile<false, false, true, 0, 1>, hf2d_lean_tile<false, true, true, 0, 1>,
      hf2d_lean_tile<true, true, true, 0, 1>},
     {hf2d_lean_tile<false, false, true, 0, 2>, hf2d_lean_tile<false, true, true, 0, 2>,
      hf2d_lean_tile<true, true, true, 0, 2>}}};
static const TileFxK kTileFx[2][2][3] = {
    {{hf2d_lean_tile_fx<false, false, false, 1>, hf2d_lean_tile_fx<false, true, false, 1>,
      hf2d_lean_tile_fx<true, true, false, 1>},
     {hf2d_lean_tile_fx<false, false, false, 2>, hf2d_lean_tile_fx<false, true, false, 2>,
      hf2d_lean_tile_fx<true, true, false, 2>}},
    {{hf2d_lean_tile_fx<false, false, true, 1>, hf2d_lean_tile_fx<false, true, true, 1>,
      hf2d_lean_tile_fx<true, true, true, 1>},
     {hf2d_lean_tile_fx<false, false, true, 2>, hf2d_lean_tile_fx<false, true, true, 2>,
      hf2d_lean_tile_fx<true, true, true, 2>}}};
static const TileTrK kTileTr[2][2] = {{hf2d_lean_tile_tr<false, 1>, hf2d_lean_tile_tr<false, 2>},
                                      {hf2d_lean_tile_tr<true, 1>, hf2d_lean_tile_tr<true, 2>}};
// single gas, small workgroups: [0: 128 threads, 1: 64][cells per thread - 1][variant]
#define HF2D_NT_ROW(K, NT, CPT) {K<false, false, NT, CPT>, K<false, true, NT, CPT>, K<true, true, NT, CPT>}
static const TileK kTileNt[2][2][3] = {{HF2D_NT_ROW(hf2d_lean_tile_nt, 128, 1), HF2D_NT_ROW(hf2d_lean_tile_nt, 128, 2)},
                                       {HF2D_NT_ROW(hf2d_lean_tile_nt, 64, 1), HF2D_NT_ROW(hf2d_lean_tile_nt, 64, 2)}};
static const TileFxK kTileFxNt[2][2][3] = {
    {HF2D_NT_ROW(hf2d_lean_tile_fx_nt, 128, 1), HF2D_NT_ROW(hf2d_lean_tile_fx_nt, 128, 2)},
    {HF2D_NT_ROW(hf2d_lean_tile_fx_nt, 64, 1), HF2D_NT_ROW(hf2d_lean_tile_fx_nt, 64, 2)}};
#undef HF2D_NT_ROW
static const TileTrK kTileTrNt[2][2] = {{hf2d_lean_tile_tr_nt<128, 1>, hf2d_lean_tile_tr_nt<128, 2>},
                                        {hf2d_lean_tile_tr_nt<64, 1>, hf2d_lean_tile_tr_nt<64, 2>}};
// threads per workgroup of the inviscid tile kernel: 256, or 128 / 64 (single gas)
inline int tile_nt(int want, bool sg) { return sg && (want == 128 || want == 64) ? want : BLOCK; }
// the kernel of a family for nt threads per workgroup (below 256: the
// single-gas small-workgroup tables), cpt cells per thread and variant var
inline TileK tile_kernel(int nt, bool sg, int cpt, int var) {
  return nt == BLOCK ? kTile[sg][cpt - 1][var] : kTileNt[nt == 128 ? 0 : 1][cpt - 1][var];
}
inline TileFxK tile_fx_kernel(int nt, bool sg, int cpt, int var) {
  return nt == BLOCK ? kTileFx[sg][cpt - 1][var] : kTileFxNt[nt == 128 ? 0 : 1][cpt - 1][var];
}
inline TileTrK tile_tr_kernel(int nt, bool sg, int cpt) {
  return nt == BLOCK ? kTileTr[sg][cpt - 1] : kTileTrNt[nt == 128 ? 0 : 1][cpt - 1];
}

// slots per thread of the batched staging for tile T (single gas), 0 where
// the kernel of nt threads and cpt cells per thread stages with the loop
inline int tile_stage_k(const LeanTile& T, int nt, int cpt) {
  const int K = (T.NC + nt - 1) / nt;
  return K <= lean_stage_kmax(nt, cpt) ? K : 0;
}
int lean_tile_stage_kmax(int nt, int cpt) {
  return (nt == BLOCK || nt == 128 || nt == 64) && (cpt == 1 || cpt == 2) ? lean_stage_kmax(nt, cpt) : 0;
}

// Cp_air(xv[t]) as the single-gas tile kernels evaluate it: the pack's AirTable
// through air_table_issue / air_table_write into LDS, then air_table_eval
// (mode 1) or table_eval on the pack (mode 0).  One workgroup of one wave.
__global__ __launch_bounds__(WAVE) void hf2d_air_table_probe(const SpeciesProps* sp, const real* xv, real* out, int n,
                                                             int table) {
  extern __shared__ double lds8[];
  AirTable* tab = reinterpret_cast<AirTable*>(lds8);
  air_table_write(tab, air_table_issue(sp));
  __syncthreads();
  const int t = (int)threadIdx.x;
  if (t < n) out[t] = table ? air_table_eval(*tab, xv[t]) : table_eval(sp->Cp[H_AIR], xv[t]);
}

std::pair<std::vector<double>, int> air_table_probe(const std::vector<double>& x, const std::vector<double>& y,
                                                    const std::vector<double>& xv) {
  if (x.size() != y.size() || x.size() > (size_t)MAX_TABLE_PTS) throw std::runtime_error("air_table_probe: table size");
  if (xv.size() > (size_t)WAVE) throw std::runtime_error("air_table_probe: at most 64 values per call");
  SpeciesDev sd;
  sd.sp.R[H_AIR] = 287.0;
  TableData& t = sd.sp.Cp[H_AIR];
  t.n = (int)x.size();
  for (int k = 0; k < MAX_TABLE_PTS; k++) {
    t.x[k] = k < t.n ? x[k] : 0.0;
    t.y[k] = k < t.n ? y[k] : 0.0;
  }
  sd.air = air_table_build(sd.sp);
  const int n = (int)xv.size();
  std::vector<real> hx(xv.begin(), xv.end()), ho(WAVE, (real)0);
  hx.resize(WAVE, (real)0);
  SpeciesDev* dsd = nullptr;
  real* dx = nullptr;
  HIP_CHECK(hipMalloc((void**)&dsd, sizeof(SpeciesDev)));
  if (hipMalloc((void**)&dx, 2 * WAVE * sizeof(real)) != hipSuccess) {
    (void)hipFree(dsd);
    throw std::runtime_error("air_table_probe: hipMalloc");
  }
  hipError_t e = hipMemcpy(dsd, &sd, sizeof(SpeciesDev), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(dx, hx.data(), WAVE * sizeof(real), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(hf2d_air_table_probe, dim3(1), dim3(WAVE), AIR_TABLE_LDS_BYTES, 0, &dsd->sp, dx, dx + WAVE, n,
                       sd.air.mode);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpy(ho.data(), dx + WAVE, WAVE * sizeof(real), hipMemcpyDeviceToHost);
  (void)hipFree(dx);
  (void)hipFree(dsd);
  if (e != hipSuccess) throw std::runtime_error(std::string("air_table_probe: ") + hipGetErrorString(e));
  return {std::vector<double>(ho.begin(), ho.begin() + n), sd.air.mode};
}

using LeanEulerK =void (*)(StepParams, LeanSoA, long, long, DevScalars*, int, int, int, ResidualPack*);
// [residual][first lean step: from the generic arrays]
static const LeanEulerK kLeanEuler[2][2] = {{hf2d_lean_euler<false, false>, hf2d_lean_euler<false, true>},
                                            {hf2d_lean_euler<true, false>, hf2d_lean_euler<true, true>}};

void DeviceSolver::lean_materialize() {
  p2p_complete();
  Impl& m = *impl;
  StepParams P = make_params(last_iter + iter);
  P.nx = h.nx;
  P.ny = h.ny;
  LeanSoA L = m.lean_view(h, sbuf, abuf, dsbuf, pbuf, false);
  SoA g = m.view(h, sbuf, abuf, dsbuf, pbuf);
  const unsigned nb = (unsigned)((h.N + BLOCK - 1) / BLOCK);
  hipLaunchKernelGGL(hf2d_lean_materialize, dim3(nb), dim3(BLOCK), 0, m.stream, P, L, g, 0L, h.N);
  HIP_CHECK(hipGetLastError());
  lean_state = 0;
}

// Inviscid lean tile step (lean_tile.hpp).
DeviceSolver::StepDone DeviceSolver::step_tile(StepCtx& c) {
  Impl& m = *impl;
  hipStream_t st = m.stream;
  StepParams& P = c.P;   // (the tile kernel's own flags are set below)
  const bool want_res = c.want_res;
  const int slot = c.slot, slot_next = c.slot_next, serial = c.serial;
  LeanSoA L = m.lean_view(h, sbuf, abuf, dsbuf, pbuf, false);
  P.skip_same = tile_skip_same ? 1 : 0;
  P.dt_read = dt_read_mode == 1 ? 1 : 0;
  // two cells per thread unless that leaves fewer than ~2 workgroups per CU
  // (small strips of a multi-GPU run)
  // (256-thread tiles only: the small-workgroup geometries are explicit
  // choices of the autotune)
  const bool sg = lean_sg && lean_sg_ok;
  const int nt = tile_nt(lean_nt, sg);
  int cpt = lean_cpt == 2 ? 2 : 1;
  if (cpt == 2 && nt == BLOCK) {
    const LeanTile T2 = lean_tile_geom(P.i1 - P.i0, P.ny, BLOCK, lean_tj, 2);
    if ((long)T2.nbi * T2.nbj < 2L * cu_count) cpt = 1;
  }
  LeanTile T = lean_tile_geom(P.i1 - P.i0, P.ny, nt, lean_tj, cpt);
  T.stage = sg ? tile_stage_k(T, nt, cpt) : 0;
  const unsigned ntile = (unsigned)(T.nbi * T.nbj);
  T.table = sg ? air_table_mode : 0;
  // (single gas: the AirTable behind the fields, in either mode)
  size_t shmem = sg ? air_table_lds_offset(T.NC) + AIR_TABLE_LDS_BYTES : (size_t)lean_tile_fields(sg) * T.NC * sizeof(real);
  if (lean_wgcu > 0)   // cap the resident workgroups per CU through the LDS request (160 KB per CU)
    shmem = std::max(shmem, (size_t)((LDS_PER_CU / lean_wgcu - 1024) & ~255));
  // an armed recorder needs T of every step, which the plain variant does
  // not store: where R is constant over a tile step (single gas, or no
  // reactions) the recorder forms it from p, R, rho; a reacting mixture
  // runs the output variant instead
  const bool rec_out = (probes_live() || stats_live() || frames_live()) && !sg && P.chem_model != NO_REACTIONS;
  const bool out = step_outputs || want_res || rec_out;
  // staggered start only for a grid that is resident at once (<= 4 dispatch
  // rounds: measured 1.5 us faster on the headline grid; the 4000x1000 triple
  // point, dispatched in ~15 waves, ran 350 -> 550 us with it)
  P.stagger_wgs = cu_count > 0 ? cu_count : 256;
  P.stagger = ntile <= 4u * (unsigned)P.stagger_wgs && nt == BLOCK ? tile_stagger : 0;
  // (64-thread tiles, the whole grid resident at once: a linear start ramp
  // over the grid of 2 / 4 / 7 / 10 us measured 4.7 / 6.4 / 15 / 27 %
  // slower than none, profiles/r04_start.md)
  // multi-GPU: exchange fused into the tile kernel (no separate exchange launch)
  const bool fx_step = m.p2p.on && p2p_fuse && !lean_has_cauchy_x;
  FusedX X = fx_step ? fused_args() : FusedX{};
  // lagged dt: the fused tail waits for the two neighbours only; the dt
  // MIN follows in the next fused step's first workgroup or in
  // hf2d_p2p_complete before any other consumer (fx_pending)
  X.defer = fx_step && P.lag_dt ? 1 : 0;
  lean_tile_last.nt = nt;
  lean_tile_last.cpt = cpt;
  lean_tile_last.TI = T.TI;
  lean_tile_last.TJ = T.TJ;
  lean_tile_last.nbi = T.nbi;
  lean_tile_last.nbj = T.nbj;
  lean_tile_last.stage = T.stage;
  lean_tile_last.table = T.table;
  // (the stagger block is compiled into the single-gas two-cell 256-thread plain kernel only)
  lean_tile_last.stagger = HF2D_TILE_STAGGER && sg && cpt == 2 && !fx_step && nt == BLOCK ? P.stagger : 0;
  lean_tile_last.fx = fx_step ? 1 : 0;
  lean_tile_last.seen = c.tile_prev.nt == nt && c.tile_prev.cpt == cpt ? c.tile_prev.seen : 0;
  // RCCL / in-process transports: edge tiles first, their halo on the comm
  // stream while the interior tiles compute, then the dt MIN
  // (the decision must be the same on every rank -- the exchange sequence
  // differs -- so a strip too narrow to split runs all its tiles at once)
  const bool split = comm_overlap && !fx_step && !m.p2p.on && (m.comm || m.local) && m.nranks > 1 &&
                     !want_res && !out && !tile_trace;
  if (split) {
    lean_tile_last.seen |= 1;   // (the part launches are plain steps)
    lean_T_stored = false;
    overlap_streams();
    const bool parts = T.nbi >= 3;
    const unsigned ne = parts ? (unsigned)(2 * T.nbj) : ntile, ni = parts ? (unsigned)((T.nbi - 2) * T.nbj) : 0u;
    const TileK pk = tile_kernel(nt, sg, cpt, 0);
    hipLaunchKernelGGL(pk, dim3(ne), dim3(nt), shmem, st, P, L, T, m.sc, slot, slot_next, serial, m.partials,
                       parts ? 1 : 0);
    HIP_CHECK(hipGetLastError());
    flip_state();   // the new state is this step's output arrays
    HIP_CHECK(hipEventRecord(m.ev_edge, st));
    // interior tiles in flight before the (possibly host-blocking) exchange
    // is issued; they write neither the edge columns nor the ghost columns
    if (ni > 0)
      hipLaunchKernelGGL(pk, dim3(ni), dim3(nt), shmem, st, P, L, T, m.sc, slot, slot_next, serial, m.partials,
                         2);
    HIP_CHECK(hipGetLastError());
    overlap_exchange(CpuSolver::HALO_LEAN, slot_next);
    return {ntile, nt / WAVE, true};
  }
  // variant: 0 plain, 1 outputs, 2 residual (all variants of one step use
  // the cpt the tile geometry was built for)
  const int var = want_res ? 2 : out ? 1 : 0;
  lean_tile_last.var = var;
  lean_tile_last.seen |= 1 << var;
  lean_T_stored = var != 0;
  if (tile_trace && var == 0 && !fx_step)
    hipLaunchKernelGGL(tile_tr_kernel(nt, sg, cpt), dim3(ntile), dim3(nt), shmem, st, P, L, T, m.sc, slot, slot_next,
                       serial, m.partials, tile_trace);
  else if (fx_step) {
    // the fused tail folds every rank's dt into the next slot's word
    // (fx_tail): the next fused step reads that one word (not when the
    // fold is deferred, lagged dt)
    const bool word = dt_read_mode >= 1 && !X.defer;
    if (word && c.dt_word_ok) P.dt_read = 2;
    lean_tile_last.dt_read = P.dt_read;
    hipLaunchKernelGGL(tile_fx_kernel(nt, sg, cpt, var), dim3(ntile), dim3(nt), shmem, st, P, L, T, m.sc, slot,
                       slot_next, serial, m.partials, fx_device(X));
    dt_word_valid = word;
    fx_pending = true;   // exchanged inside the tile kernel
  } else {
    // single GPU, last step of the host call: the scalars go to the host
    // mirror from the kernel's own tail (host_tail)
    const bool mirror = var == 1 && step_outputs && !tile_trace && host_tail && m.nranks == 1 && !m.local && !m.p2p.on;
    if (mirror) {
      P.host_sc = m.sc_host;
      P.host_done = m.host_done;
    }
    // dt read of the tile kernel (StepParams::dt_read): with dt_read_mode
    // 2 every step's last workgroup folds the shards into the word and the
    // next step's workgroups read that one word
    const bool fold = dt_read_mode == 2 && !tile_trace && m.nranks == 1 && !m.local && !m.p2p.on;
    P.dt_read = (fold && c.dt_word_ok) ? 2 : dt_read_mode == 1 ? 1 : 0;
    if (fold) {
      P.dt_fold = 1;
      P.host_done = m.host_done;
    }
    lean_tile_last.dt_read = P.dt_read;
    hipLaunchKernelGGL(tile_kernel(nt, sg, cpt, var), dim3(ntile), dim3(nt), shmem, st, P, L, T, m.sc, slot, slot_next,
                       serial, m.partials, 0);
    m.sc_mirrored = mirror;
    dt_word_valid = fold;
  }
  HIP_CHECK(hipGetLastError());
  flip_state();
  return {ntile, nt / WAVE, fx_step};
}

// Flat lean Euler step (the first lean step, or every one without lean_tile).
DeviceSolver::StepDone DeviceSolver::step_lean_flat(const StepCtx& c) {
  Impl& m = *impl;
  const bool fromg = lean_state == 0;
  LeanSoA L = m.lean_view(h, sbuf, abuf, dsbuf, pbuf, fromg);
  hipLaunchKernelGGL(kLeanEuler[c.want_res][fromg], dim3(c.nblk), dim3(BLOCK), 0, m.stream, c.P, L, c.c0, c.c1, m.sc,
                     c.slot, c.slot_next, c.serial, m.partials);
  HIP_CHECK(hipGetLastError());
  flip_state();
  lean_state = 1;
  lean_T_stored = true;   // (the flat kernel always writes the output-only fields)
  return {c.nblk, BLOCK / WAVE, false};
}

// One traced lean tile step (after `steps` untraced ones): per workgroup the
// phase clocks of lean_tile_body<TR> (TILE_TRACE_WORDS words each, tile order).
std::vector<unsigned long long> DeviceSolver::trace_tile(int steps) {
  if (!lean_ok || cs.cfg.ProblemType == SM_NS || !lean_tile) throw std::runtime_error("trace_tile: lean tile steps only");
  flush_pending();
  const bool g = use_graph;
  use_graph = false;
  if (steps > 0) run_steps(steps);
  const int cpt = lean_cpt == 2 ? 2 : 1;
  const LeanTile T = lean_tile_geom(gi1 - gi0, h.ny, tile_nt(lean_nt, lean_sg && lean_sg_ok), lean_tj, cpt);
  const long n = (long)T.nbi * T.nbj * TILE_TRACE_WORDS * 2;   // room for either cpt
  tile_trace = impl->mem.alloc<unsigned long long>(n);
  try {
    run_steps(2);   // the last step of run_steps stores the output fields (not traced)
    synchronize();
  } catch (...) {
    tile_trace = nullptr;
    use_graph = g;
    throw;
  }
  std::vector<unsigned long long> out(n);
  HIP_CHECK(hipMemcpy(out.data(), tile_trace, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  tile_trace = nullptr;
  use_graph = g;
  while (!out.empty() && out.back() == 0) out.pop_back();
  out.resize((out.size() + TILE_TRACE_WORDS - 1) / TILE_TRACE_WORDS * TILE_TRACE_WORDS);
  return out;
}

}  // namespace hf2d
