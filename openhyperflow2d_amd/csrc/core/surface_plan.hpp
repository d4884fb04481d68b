// Per-node wall surface distributions (record_surface): p, Cp, T, the wall
// shear, Cf, the wall heat flux and St of every wall node after every sampled
// step: the un-folded form of the load recorder (load_plan.hpp) and of the wall
// heat recorder (wall_heat.hpp), from the very functions they fold.
//
// A node is a set, non-solid cell that carries CT_WALL_NO_SLIP or CT_WALL_LAW,
// or that has a CT_SOLID cell among its in-grid 4-neighbours (the slip surface
// of an Euler body, which the load integrals skip).  Nodes are listed in
// (i outer, j inner) order; with boxes, the lists of the boxes one after the
// other (in_box, as build_load_plan), a node inside two boxes in both.
//
// Which neighbour gives a friction term its sign, with which area and sign a
// node enters the pressure and friction folds: wall_node_terms, the one
// function build_load_plan and this plan both call.
//
// The ten values of a node (SURFACE_VARS), all in `real`, one operation per
// statement, IEEE `/`, nothing to contract:
//   p, T            the node's p and Tg
//   Cp              (p - Pg) / cp_den                       (wall_heat_x_term's line)
//   tau_x, tau_y    load_term(LK_FX | LK_FY, 1, ...) with the load plan's
//                   neighbour; +0.0 where the load plan has no friction term
//   Cf_x, Cf_y      tau / cp_den
//   q_y, q_x        wall_heat_q over dy, dx; +0.0 unless the node is
//                   CT_WALL_NO_SLIP with N1..N4 inside the grid
//   St              q_y / st_den
// Every (variable, node) entry has the running statistics of wall_heat.hpp
// (wall_heat_stat on a StatsScalars tick of the recorder's own).
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "load_plan.hpp"
#include "wall_heat.hpp"

namespace hf2d {

constexpr int SURFACE_NVARS = 10;
enum SurfaceVar { SV_P = 0, SV_CP, SV_T, SV_TAUX, SV_TAUY, SV_CFX, SV_CFY, SV_QY, SV_QX, SV_ST };

// flags of a node (the table's `flags`: bits 0..2) and what its values read
enum SurfaceNodeBit : uint8_t {
  SN_NO_SLIP = 1,   // CT_WALL_NO_SLIP
  SN_LAW = 2,       // CT_WALL_LAW
  SN_SOLID_NB = 4,  // a CT_SOLID cell among the in-grid 4-neighbours
  SN_FRIC_X = 8,    // the load plan has an x friction term for the node
  SN_FRIC_Y = 16,   // ... a y friction term
  SN_HEAT = 32,     // CT_WALL_NO_SLIP with N1..N4 inside the grid
};
// what a needed cell is needed for (SurfacePlan::mask)
enum SurfaceCellBit : uint8_t {
  SC_NODE = 1,   // a node: the values of the fill
  SC_U = 2,      // an x friction neighbour: U
  SC_V = 4,      // a y friction neighbour: V
  SC_LAM = 8,    // one of a node's N1..N4: lam + lam_t
};
// planes of the scratch array, [SURFACE_PLANES][ncells]
enum SurfacePlane { SP_P = 0, SP_T, SP_SL, SP_MU, SP_MUT, SP_DUDY, SP_DVDX, SP_U, SP_V, SURFACE_PLANES };
constexpr int SURFACE_IDX = 7;   // per list position: the node, its x and y friction neighbours, N1..N4

struct SurfaceOpts {
  bool all = true;               // every node, no box test (boxes=None)
  std::vector<LoadBox> boxes;
  int cp_flow = 0;               // 1-based flow of Cp, Cf and St
  int every = 1;
  long capacity = 1024;          // 0: statistics only
  bool statistics = true, step_weight = false;
};

struct SurfacePlan {
  int nboxes = 0;                // lists: the boxes, or 1
  WallHeatConst K;
  std::vector<long> cells;       // unique needed cells (local index)
  std::vector<uint8_t> mask;     // [ncells] SurfaceCellBit
  std::vector<int> idx;          // [nnodes][SURFACE_IDX] indices into cells (the node's own where there is none)
  std::vector<uint8_t> bits;     // [nnodes] SurfaceNodeBit
  // the static node table
  std::vector<int> ni, nj;
  std::vector<real> x, y, face_x, face_y, fric_x, fric_y;
  std::vector<long> box_off;     // [nboxes + 1]
  long nnodes() const { return (long)bits.size(); }
  size_t nentries() const { return (size_t)SURFACE_NVARS * bits.size(); }
  long ncells() const { return (long)cells.size(); }
  bool friction() const {
    for (uint8_t b : bits)
      if (b & (SN_FRIC_X | SN_FRIC_Y)) return true;
    return false;
  }
};

// What surface_history() returns: an entry is one variable of one node, a row
// [SURFACE_NVARS][nnodes].
struct SurfaceHistory : SampledHistory {
  long nnodes = 0;
};

// The ten values of one node from what a download after the step holds.
struct SurfaceIn {
  real p, Tg, mu, mu_t, dUdy, dVdx;   // of the node
  real U_nb, V_nb;                     // of its x / y friction neighbour
  real sl[5];                          // lam + lam_t of the node and N1..N4
};
HF_HD inline void surface_values(const WallHeatConst& K, int bits, const SurfaceIn& a, real out[SURFACE_NVARS]) {
  out[SV_P] = a.p;
  const real dp = a.p - K.Pg;
  out[SV_CP] = dp / K.cp_den;
  out[SV_T] = a.Tg;
  real tx = 0, ty = 0, cfx = 0, cfy = 0;
  if (bits & SN_FRIC_X) {
    tx = load_term(LK_FX, (real)1, (real)0, a.mu, a.mu_t, a.dUdy, a.U_nb);
    cfx = tx / K.cp_den;
  }
  if (bits & SN_FRIC_Y) {
    ty = load_term(LK_FY, (real)1, (real)0, a.mu, a.mu_t, a.dVdx, a.V_nb);
    cfy = ty / K.cp_den;
  }
  out[SV_TAUX] = tx;
  out[SV_TAUY] = ty;
  out[SV_CFX] = cfx;
  out[SV_CFY] = cfy;
  real qy = 0, qx = 0, st = 0;
  if (bits & SN_HEAT) {
    const real lam_eff = wall_heat_lam_eff(a.sl[0], a.sl[1], a.sl[2], a.sl[3], a.sl[4]);
    qy = wall_heat_q(K, lam_eff, a.Tg, K.dy);
    qx = wall_heat_q(K, lam_eff, a.Tg, K.dx);
    st = qy / K.st_den;
  }
  out[SV_QY] = qy;
  out[SV_QX] = qx;
  out[SV_ST] = st;
}

// ... of list position n from the scratch planes (sc: [SURFACE_PLANES][nc])
HF_HD inline void surface_node(const WallHeatConst& K, const int* idx, const uint8_t* bits, const real* sc, long nc,
                               long n, real out[SURFACE_NVARS]) {
  const int* c = idx + SURFACE_IDX * n;
  SurfaceIn a;
  a.p = sc[SP_P * nc + c[0]];
  a.Tg = sc[SP_T * nc + c[0]];
  a.mu = sc[SP_MU * nc + c[0]];
  a.mu_t = sc[SP_MUT * nc + c[0]];
  a.dUdy = sc[SP_DUDY * nc + c[0]];
  a.dVdx = sc[SP_DVDX * nc + c[0]];
  a.U_nb = sc[SP_U * nc + c[1]];
  a.V_nb = sc[SP_V * nc + c[2]];
  a.sl[0] = sc[SP_SL * nc + c[0]];
  for (int q = 1; q < 5; q++) a.sl[q] = sc[SP_SL * nc + c[2 + q]];
  surface_values(K, bits[n], a, out);
}

inline void check_surface(const SurfaceOpts& o) {
  if ((int)o.boxes.size() > LOAD_MAX)
    throw std::invalid_argument("record_surface: " + std::to_string(o.boxes.size()) + " boxes, at most " +
                                std::to_string(LOAD_MAX));
  for (const LoadBox& b : o.boxes)
    for (double v : b)
      if (!std::isfinite(v)) throw std::invalid_argument("record_surface: a box holds a number that is not finite");
  if (o.every < 1) throw std::invalid_argument("record_surface: every must be at least 1");
  if (o.capacity < 0) throw std::invalid_argument("record_surface: capacity must not be negative");
  if (o.capacity == 0 && !o.statistics)
    throw std::invalid_argument("record_surface: capacity 0 keeps statistics only, and statistics are off");
}

// The plan over the whole field J (one solver, not a strip); local cell of
// global (i, j): (i + l_off) * ny + j.  std::invalid_argument: the options
// (check_surface), a flow index the case does not have, a ring of more than
// 2^31 entries.
inline SurfacePlan build_surface_plan(const Case& cs, const Field& J, const SurfaceOpts& o, int l_off = 0) {
  check_surface(o);
  const Config& C = cs.cfg;
  SurfacePlan P;
  if (!wall_heat_consts(cs, o.cp_flow, P.K))
    throw std::invalid_argument("record_surface: Cp flow index " + std::to_string(o.cp_flow) + " outside the case's " +
                                std::to_string(cs.flows2d.size()) + " flows");
  P.nboxes = o.all ? 1 : (int)o.boxes.size();
  const real dx_out = (C.dx * C.MaxX) / (C.MaxX - 1);
  const real dy_out = (C.dy * C.MaxY) / (C.MaxY - 1);
  std::vector<int> slot((size_t)J.nx * J.ny, -1);
  auto need = [&](int i, int j, uint8_t why) {
    int& s = slot[(size_t)i * J.ny + j];
    if (s < 0) {
      s = (int)P.cells.size();
      P.cells.push_back((long)(i + l_off) * J.ny + j);
      P.mask.push_back(0);
    }
    P.mask[s] |= why;
    return s;
  };
  auto solid = [&](int i, int j) { return J.in(i, j) && J.at(i, j).is(CT_SOLID); };
  P.box_off.push_back(0);
  for (int b = 0; b < P.nboxes; b++) {
    for (int i = 0; i < J.nx; i++)
      for (int j = 0; j < J.ny; j++) {
        const CellRecord& n = J.at(i, j);
        if (!n.is(CT_NODE_IS_SET) || n.is(CT_SOLID)) continue;
        uint8_t bits = 0;
        if (n.is(CT_WALL_NO_SLIP)) bits |= SN_NO_SLIP;
        if (n.is(CT_WALL_LAW)) bits |= SN_LAW;
        if (solid(i - 1, j) || solid(i + 1, j) || solid(i, j - 1) || solid(i, j + 1)) bits |= SN_SOLID_NB;
        if (!bits) continue;
        if (!o.all) {
          const LoadBox& q = o.boxes[b];
          if (!in_box(C, i, j, (real)q[0], (real)q[1], (real)q[2], (real)q[3])) continue;
        }
        WallNodeTerms t;
        if (bits & (SN_NO_SLIP | SN_LAW)) t = wall_node_terms(C, J, i, j);
        int c[SURFACE_IDX];
        c[0] = need(i, j, SC_NODE);
        for (int q = 1; q < SURFACE_IDX; q++) c[q] = c[0];
        if (t.has_fx) {
          bits |= SN_FRIC_X;
          c[1] = need(t.fx_i, t.fx_j, SC_U);
        }
        if (t.has_fy) {
          bits |= SN_FRIC_Y;
          c[2] = need(t.fy_i, t.fy_j, SC_V);
        }
        if (bits & SN_NO_SLIP) {
          const int q4[4][2] = {{i - n.idXl, j}, {i + n.idXr, j}, {i, j + n.idYu}, {i, j - n.idYd}};
          bool in = true;
          for (const auto& a : q4) in = in && J.in(a[0], a[1]);
          if (in) {
            bits |= SN_HEAT;
            for (int q = 0; q < 4; q++) c[3 + q] = need(q4[q][0], q4[q][1], SC_LAM);
          }
        }
        P.idx.insert(P.idx.end(), c, c + SURFACE_IDX);
        P.bits.push_back(bits);
        P.ni.push_back(i);
        P.nj.push_back(j);
        const real xi = i * dx_out, yj = dy_out * j;   // (the field dump's columns: plt_row)
        P.x.push_back(xi * 1.e3);
        P.y.push_back(yj * 1.e3);
        P.face_x.push_back(t.face_x);
        P.face_y.push_back(t.face_y);
        P.fric_x.push_back(t.fric_x);
        P.fric_y.push_back(t.fric_y);
      }
    P.box_off.push_back(P.nnodes());
  }
  const double ring = (double)o.capacity * (double)SURFACE_NVARS * (double)P.nnodes();
  if (ring > 2147483648.0)
    throw std::invalid_argument("record_surface: a ring of " + std::to_string(o.capacity) + " x " +
                                std::to_string(SURFACE_NVARS) + " x " + std::to_string(P.nnodes()) +
                                " entries, at most 2^31");
  return P;
}

// The scratch planes from the records (Case.surface): what a backend writes
// from its own arrays after a step.  sc: [SURFACE_PLANES][ncells]
inline void surface_scratch_of_records(const SurfacePlan& P, const Field& J, int l_off, real* sc) {
  const long nc = P.ncells();
  for (long k = 0; k < nc; k++) {
    const long c = P.cells[k];
    const CellRecord& n = J.at((int)(c / J.ny) - l_off, (int)(c % J.ny));
    sc[SP_P * nc + k] = n.p;
    sc[SP_T * nc + k] = n.Tg;
    sc[SP_SL * nc + k] = n.lam + n.lam_t;
    sc[SP_MU * nc + k] = n.mu;
    sc[SP_MUT * nc + k] = n.mu_t;
    sc[SP_DUDY * nc + k] = n.dUdy;
    sc[SP_DVDX * nc + k] = n.dVdx;
    sc[SP_U * nc + k] = n.U;
    sc[SP_V * nc + k] = n.V;
  }
}

// One sample from the scratch planes: the ring row (row: [SURFACE_NVARS][nn],
// or null) and the statistics (stat: m, M, peak, peak_time [SURFACE_NVARS * nn]
// each, or null) on the tick's weights.
inline void surface_sample(const SurfacePlan& P, const real* sc, real* row, double* stat, const StatsScalars& tk,
                           double t) {
  const long nn = P.nnodes(), nc = P.ncells();
  const size_t ne = (size_t)SURFACE_NVARS * nn;
  for (long n = 0; n < nn; n++) {
    real out[SURFACE_NVARS];
    surface_node(P.K, P.idx.data(), P.bits.data(), sc, nc, n, out);
    for (int v = 0; v < SURFACE_NVARS; v++) {
      const size_t e = (size_t)v * nn + n;
      if (row) row[e] = out[v];
      if (stat)
        wall_heat_stat(tk.w, tk.r, t, tk.samples == 1, (double)out[v], stat[e], stat[ne + e], stat[2 * ne + e],
                       stat[3 * ne + e]);
    }
  }
}

// Ring and statistics -> SurfaceHistory, oldest first (sampled_history_fill).
template <class TimeOf>
inline SurfaceHistory surface_history_from(const SurfacePlan& P, const SurfaceOpts& o, const SampledRing& r,
                                           TimeOf time_of) {
  SurfaceHistory H;
  H.nnodes = P.nnodes();
  sampled_history_fill(H, r, o.capacity, P.nentries(), o.statistics, time_of);
  return H;
}

}  // namespace hf2d
