// Per-step monitor-point recorder (K8 time series): after every step one
// 64-lane workgroup appends a row (p, T, rho, U, V) per probe cell, and the
// step's time, to a device ring buffer.  It runs on the solver's stream as
// the step's last launch, so it is captured into the step graphs; the ring
// index is a device counter the kernel advances itself (a replayed graph
// carries no host values).
//
// Every value is bit for bit what a download after that step yields.  The
// kernel reads the representation that is authoritative after the step:
//   PR_GATHER  generic record, or the lean inviscid arrays (lean_euler.hpp)
//              after a step that stored T: rho, U, V, T, p are stored per cell
//   PR_LEAN    lean inviscid arrays after a plain tile step, which stores no
//              T: T = p / R / rho as lean_cell forms it.  Only where R does
//              not change over a tile step (single gas, or no reactions); for
//              a reacting mixture the solver runs the tile kernel's output
//              variant while a recorder is armed (PR_GATHER)
//   PR_SGL /   lean N-S state (lean_ns.hpp): Sp^{m+1} and the level-m
//   PR_SGT     primitives; the row is the own-cell part of the fill F_{m+1}
//              the materialise would run (fill_compute through ProbeOwnIO:
//              U, V, T, p of a node depend on no neighbour)
//   PR_MECH    lean mechanism state (lean_mech.hpp): T and p of the new level
//              are stored; U, V by fill_node_pre / fill_node_wall from
//              Sp^{m+1} and the lagged velocity, as mech_state_node
// The step kernels and their argument blocks are untouched.
#pragma once

#include "lean_mech.hpp"

namespace hf2d {

// fill_compute() accessor of one node without neighbours over the SoA view
// the materialise fill reads (DeviceSolver::lns_materialize): every neighbour
// resolves to the node itself, so the fluxes, gradients and turbulence
// sources it yields are meaningless and discarded; S, U, V, T, p are the
// fill's (as LnsOwnIO, whose U, V, T, k feed dt_{m+1}).
struct ProbeOwnIO {
  static constexpr int TURB_SET = 0;   // the turbulence model touches none of the row's values
  const SoA& s;
  long N, idx;
  HF_HD ProbeOwnIO(const SoA& s_, long i) : s(s_), N(s_.N), idx(i) {}
  HF_HD void set_nb(int, int, int, int, int, int, int) {}
  HF_HD u64 CT() const { return s.CT[idx]; }
  HF_HD u64 TT() const { return s.TT[idx]; }
  HF_HD uint8_t gf() const { return s.gf ? s.gf[idx] : (uint8_t)0xff; }
  HF_HD uint8_t nb() const { return s.nb[idx]; }
  HF_HD real S(int k) const { return s.S[k * N + idx]; }
  HF_HD real Sn(int k, int) const { return s.S[k * N + idx]; }
  HF_HD real A(int) const { return 0.0; }
  HF_HD real B(int) const { return 0.0; }
  HF_HD real F(int) const { return 0.0; }
  HF_HD real Src(int) const { return 0.0; }
  HF_HD real SrcAdd(int) const { return 0.0; }
  HF_HD real Uo() const { return s.U[idx]; }
  HF_HD real Vo() const { return s.V[idx]; }
  HF_HD real To() const { return s.Tg[idx]; }
  HF_HD real Uon(int) const { return s.U[idx]; }
  HF_HD real Von(int) const { return s.V[idx]; }
  HF_HD real Ton(int) const { return s.Tg[idx]; }
  HF_HD real p() const { return 0.0; }   // rewritten by fill_node before any use
  HF_HD real kk() const { return s.kk[idx]; }
  HF_HD real R() const { return s.R[idx]; }
  HF_HD real CP() const { return s.CP[idx]; }
  HF_HD real lam() const { return s.lam[idx]; }
  HF_HD real mu() const { return s.mu[idx]; }
  HF_HD real Diff() const { return 0.0; }
  HF_HD real mu_t() const { return s.mu_t[idx]; }
  HF_HD real lam_t() const { return 0.0; }
  HF_HD real l_min() const { return s.l_min[idx]; }
  HF_HD real y_plus() const { return s.y_plus[idx]; }
  HF_HD real Re_local() const { return 0.0; }
  HF_HD real BGX() const { return s.BGX[idx]; }
  HF_HD real BGY() const { return s.BGY[idx]; }
  HF_HD real Tf() const { return 0.0; }
  HF_HD real Y(int) const { return 0.0; }
  HF_HD real grad(int) const { return 0.0; }
  HF_HD real Ys(int) const { return 0.0; }
  HF_HD real Ysn(int, int) const { return 0.0; }
};

// Own-cell part of the materialise fill of one node into `c` (lean N-S /
// mechanism kinds; shared with the load recorder, load_history.hpp): c.S, c.U,
// c.V, and for PR_SGL / PR_SGT also c.Tg, c.p.  `s` as probe_row's.  false:
// the fill carries the node early (solid / unset: only c.S is formed).
template <int KIND>
HF_HD inline bool probe_own_cell(const StepParams& P, const SoA& s, long idx, CellLocal& c) {
  const long N = s.N;
  if (KIND == PR_MECH) {
#pragma unroll
    for (int k = 0; k < NEQ; k++) {
      c.S[k] = k < 4 ? s.S[k * N + idx] : 0.0;
      c.SrcAdd[k] = 0.0;
    }
#pragma unroll
    for (int q = 0; q < NSPEC; q++) c.Y[q] = 0.0;
    c.CT = s.CT[idx];
    c.U = s.U[idx];
    c.V = s.V[idx];
    c.k = s.kk[idx];
    c.BGX = s.BGX[idx];
    c.BGY = s.BGY[idx];
    c.Uw = c.Vw = 0.0;
    if (fill_node_pre(c)) fill_node_wall(c, P.fpa);
    return true;
  } else {
    constexpr int MODE = KIND == PR_SGT ? SK_SGT : SK_SGL;
    const int i = (int)(idx / P.ny), j = (int)(idx - (long)i * P.ny);
    ProbeOwnIO io(s, idx);
    real mY[1], mgx[1], mgy[1];
    bool early, filled;
    int neg = 0;
    (void)fill_compute<MODE, 1, ProbeOwnIO, true>(P, io, c, mY, mgx, mgy, nullptr, 0, i, j, true, &neg, &early,
                                                    &filled);
    return !early;
  }
}

// Row of one node.  `s` by kind:
//   PR_GATHER  S, U, V, Tg, p: the current arrays
//   PR_SGL/T   the materialise fill's input view (Sp^{m+1}, level-m fields)
//   PR_MECH    S = Sp^{m+1}, U / V / kk = the lagged level, Tg / p = the
//              stored state of the new level
template <int KIND>
HF_HD inline void probe_row(const StepParams& P, const SoA& s, long idx, real* row) {
  if (KIND == PR_GATHER) {
    row[0] = s.p[idx];
    row[1] = s.Tg[idx];
    row[2] = s.S[idx];
    row[3] = s.U[idx];
    row[4] = s.V[idx];
  } else if (KIND == PR_LEAN) {
    const real p = s.p[idx], rho = s.S[idx];
    row[0] = p;
    row[1] = hf_div(hf_div(p, s.R[idx]), rho);   // lean_cell's Tg
    row[2] = rho;
    row[3] = s.U[idx];
    row[4] = s.V[idx];
  } else if (KIND == PR_MECH) {
    CellLocal c;
    (void)probe_own_cell<KIND>(P, s, idx, c);
    row[0] = s.p[idx];
    row[1] = s.Tg[idx];
    row[2] = c.S[I_RHO];
    row[3] = c.U;
    row[4] = c.V;
  } else {
    CellLocal c;
    const bool early = !probe_own_cell<KIND>(P, s, idx, c);
    // (a solid / unset node is refused at arming: the fill of any other node
    // recovers U, V, T, p unless it is skipped, and a skipped node stops the
    // lean step itself, LNS_SKIP_ERR)
    row[0] = early ? s.p[idx] : c.p;
    row[1] = early ? s.Tg[idx] : c.Tg;
    row[2] = c.S[I_RHO];
    row[3] = early ? s.U[idx] : c.U;
    row[4] = early ? s.V[idx] : c.V;
  }
}

#ifdef __HIPCC__
template <int KIND>
__global__ __launch_bounds__(PROBE_MAX) void hf2d_probe_record(StepParams P, SoA s, ProbeRing r,
                                                                const DevScalars* sc) {
  const int t = (int)threadIdx.x;
  const unsigned long long n = *r.count;   // (one wavefront: every lane loads before lane 0 stores)
  const long slot = (long)(n % (unsigned long long)r.cap);
  if (t < r.n) {
    const long idx = r.idx[t];
    real row[PROBE_VARS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (idx >= 0 && idx < s.N) probe_row<KIND>(P, s, idx, row);
    real* o = r.rows + (slot * r.n + t) * PROBE_VARS;
#pragma unroll
    for (int v = 0; v < PROBE_VARS; v++) o[v] = row[v];
  }
  if (t == 0) {
    r.times[slot] = sc->time_part;
    *r.count = n + 1;
  }
}
#endif

}  // namespace hf2d
