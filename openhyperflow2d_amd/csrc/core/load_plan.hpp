// Per-step load recorder (record_loads): the body force of a box and the mass
// flow through an x cut, after every step, as the host integrals of
// postproc.cpp would give them on a field downloaded after that step.
//
// Which cell contributes to which integral, with which area and which
// sign-giving neighbour, depends only on the flags, the indices and the
// records' y: the plan lists that once, one entry per term, in the order
// x_force_terms / y_force_terms / mass_flow_rate_x push their terms.  Per box
// four lists (x pressure, x friction, y pressure, y friction), then one list
// per cut.  A backend evaluates every term after a step (load_term) and folds
// each list in list order (fold_terms' `s = 0; s += t`), so the values are
// those of the host functions bit for bit.  Both backends share the plan.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "postproc.hpp"
#include "ring_history.hpp"
#include "stepkern.hpp"

namespace hf2d {

constexpr int LOAD_MAX = 16;     // boxes, and cuts, of one recorder
constexpr int LOAD_PARTS = 4;    // Fx_p, Fx_d, Fy_p, Fy_d

enum LoadKind : uint8_t {
  LK_P = 0,    // coef * p[cell]                                   (coef: -Sp or Sp)
  LK_FX = 1,   // coef * (mu + mu_t) * |dUdy|, sign of U[cell2]    (coef: Sd)
  LK_FY = 2,   // coef * (mu + mu_t) * |dVdx|, sign of V[cell2]    (coef: -Sd)
  LK_M = 3,    // coef * S[I_RHOU][cell]                           (coef: dy or 2 pi dy y)
};

using LoadBox = std::array<double, 4>;   // x0, y0, dx, dy   (Case::x_force / y_force)
using LoadCut = std::array<double, 3>;   // x0, y0, dy       (Case::mass_flow_x)

// What load_history() returns: row k holds the values after recorded step k,
// oldest first.
struct LoadHistory {
  int nboxes = 0, ncuts = 0;
  long total = 0;                 // steps recorded since arming (rows kept: min(total, capacity))
  std::vector<double> times;      // [n] time after the step (the probe recorder's clock)
  std::vector<real> forces;       // [n][nboxes][LOAD_PARTS]
  std::vector<real> mass_flow;    // [n][ncuts]
  std::vector<long> box_terms;    // [nboxes][LOAD_PARTS] terms of each list (static)
  std::vector<long> cut_terms;    // [ncuts]
  std::vector<real> span;         // [nboxes] fold of wall_span_terms (static)
};

struct LoadPlan {
  int nboxes = 0, ncuts = 0;
  std::vector<long> cell, cell2;   // local cell of the term; the friction terms' neighbour (else the cell)
  std::vector<real> coef;
  std::vector<uint8_t> kind;
  std::vector<long> off;           // [nlists + 1] first term of each list
  std::vector<real> span;          // [nboxes] fold of wall_span_terms
  int nlists() const { return LOAD_PARTS * nboxes + ncuts; }
  long nterms() const { return (long)cell.size(); }
  bool friction() const {
    for (uint8_t k : kind)
      if (k == LK_FX || k == LK_FY) return true;
    return false;
  }
};

// One term from the values a download after the step holds: `a` is p (LK_P)
// or rho U (LK_M); mu, mu_t, g (the gradient) and nb (the neighbour's
// velocity component) are read by the friction kinds only.  The expressions
// and their association are those of x_force_terms / y_force_terms /
// mass_flow_rate_x: -(Sp * p) is (-Sp) * p exactly.
HF_HD inline real load_term(int kind, real coef, real a, real mu, real mu_t, real g, real nb) {
  if (kind == LK_P || kind == LK_M) return coef * a;
  const real tau = coef * (mu + mu_t) * std::fabs(g);
  return nb > 0 ? tau : -tau;
}

// A wall node's part in the four force lists of a box: the signed areas of its
// pressure terms (-Sp or Sp; +0.0: none), the coefficients of its friction
// terms (Sd, -Sd; +0.0: none) and the neighbour whose U / V gives each friction
// term its sign, as x_force_terms / y_force_terms choose them.  The load plan
// and the surface plan (surface_plan.hpp) both call this.
struct WallNodeTerms {
  real face_x = 0, face_y = 0, fric_x = 0, fric_y = 0;
  bool has_px = false, has_py = false, has_fx = false, has_fy = false;
  int fx_i = 0, fx_j = 0, fy_i = 0, fy_j = 0;
};
inline WallNodeTerms wall_node_terms(const Config& C, const Field& J, int i, int j) {
  WallNodeTerms t;
  const CellRecord& n = J.at(i, j);
  {   // x_force_terms
    real Sp, Sd;
    if (C.FT == FT_FLAT) {
      Sp = C.dy;
      Sd = C.dx;
    } else {
      Sp = 2 * M_PI * (j + 0.5) * C.dy * C.dy;
      Sd = 2 * M_PI * (j + 0.5) * C.dy * C.dx;
    }
    if (i > 0 && J.at(i - 1, j).is(CT_SOLID)) {
      t.has_px = true;
      t.face_x = -Sp;
    } else if (i < J.nx - 1 && J.at(i + 1, j).is(CT_SOLID)) {
      t.has_px = true;
      t.face_x = Sp;
    }
    if (j < J.ny - 1 && !J.at(i, j + 1).is(CT_SOLID)) {
      t.has_fx = true;
      t.fx_i = i;
      t.fx_j = j + 1;
    } else if (j > 0 && !J.at(i, j - 1).is(CT_SOLID)) {
      t.has_fx = true;
      t.fx_i = i;
      t.fx_j = j - 1;
    }
    if (t.has_fx) t.fric_x = Sd;
  }
  {   // y_force_terms
    real Sp, Sd;
    if (C.FT == FT_FLAT) {
      Sp = C.dx;
      Sd = C.dy;
    } else {
      Sp = 2 * M_PI * n.y * C.dx;
      Sd = 2 * M_PI * n.y * C.dy;
    }
    if (j > 0 && J.at(i, j - 1).is(CT_SOLID)) {
      t.has_py = true;
      t.face_y = -Sp;
    } else if (j < J.ny - 1 && J.at(i, j + 1).is(CT_SOLID)) {
      t.has_py = true;
      t.face_y = Sp;
    }
    if (i < J.nx - 1 && !J.at(i + 1, j).is(CT_SOLID)) {
      t.has_fy = true;
      t.fy_i = i + 1;
      t.fy_j = j;
    } else if (i > 0 && !J.at(i - 1, j).is(CT_SOLID)) {
      t.has_fy = true;
      t.fy_i = i - 1;
      t.fy_j = j;
    }
    if (t.has_fy) t.fric_y = -Sd;
  }
  return t;
}

inline void check_loads(const std::vector<LoadBox>& boxes, const std::vector<LoadCut>& cuts, long capacity) {
  if (boxes.empty() && cuts.empty()) throw std::invalid_argument("record_loads: no box and no cut");
  if ((int)boxes.size() > LOAD_MAX)
    throw std::invalid_argument("record_loads: " + std::to_string(boxes.size()) + " boxes, at most " +
                                std::to_string(LOAD_MAX));
  if ((int)cuts.size() > LOAD_MAX)
    throw std::invalid_argument("record_loads: " + std::to_string(cuts.size()) + " cuts, at most " +
                                std::to_string(LOAD_MAX));
  if (capacity < 1) throw std::invalid_argument("record_loads: capacity must be at least 1");
  for (const LoadBox& b : boxes)
    for (double v : b)
      if (!std::isfinite(v)) throw std::invalid_argument("record_loads: a box holds a number that is not finite");
  for (const LoadCut& c : cuts)
    for (double v : c)
      if (!std::isfinite(v)) throw std::invalid_argument("record_loads: a cut holds a number that is not finite");
}

// The plan over the whole field J (one solver, not a strip); local cell of
// global (i, j): (i + l_off) * ny + j.
inline LoadPlan build_load_plan(const Case& cs, const Field& J, const std::vector<LoadBox>& boxes,
                                const std::vector<LoadCut>& cuts, int l_off = 0) {
  const Config& C = cs.cfg;
  LoadPlan L;
  L.nboxes = (int)boxes.size();
  L.ncuts = (int)cuts.size();
  auto at = [&](int i, int j) { return (long)(i + l_off) * J.ny + j; };
  auto push = [&](uint8_t k, long c, long c2, real w) {
    L.kind.push_back(k);
    L.cell.push_back(c);
    L.cell2.push_back(c2);
    L.coef.push_back(w);
  };
  auto wall_in = [&](int i, int j, const LoadBox& b) {
    const CellRecord& n = J.at(i, j);
    return (n.is(CT_WALL_LAW) || n.is(CT_WALL_NO_SLIP)) && in_box(C, i, j, (real)b[0], (real)b[1], (real)b[2], (real)b[3]);
  };
  L.off.push_back(0);
  for (const LoadBox& b : boxes) {
    // x_force_terms: fp, then fd; y_force_terms: fp, then fd
    for (int part = 0; part < LOAD_PARTS; part++) {
      for (int i = 0; i < J.nx; i++)
        for (int j = 0; j < J.ny; j++) {
          if (!wall_in(i, j, b)) continue;
          const WallNodeTerms t = wall_node_terms(C, J, i, j);
          if (part == 0 && t.has_px) push(LK_P, at(i, j), at(i, j), t.face_x);
          if (part == 1 && t.has_fx) push(LK_FX, at(i, j), at(t.fx_i, t.fx_j), t.fric_x);
          if (part == 2 && t.has_py) push(LK_P, at(i, j), at(i, j), t.face_y);
          if (part == 3 && t.has_fy) push(LK_FY, at(i, j), at(t.fy_i, t.fy_j), t.fric_y);
        }
      L.off.push_back(L.nterms());
    }
    std::vector<real> t;
    wall_span_terms(cs, J, (real)b[0], (real)b[1], (real)b[2], (real)b[3], 0, J.nx, t);
    L.span.push_back(fold_terms(t));
  }
  for (const LoadCut& c : cuts) {
    const CutCells q = cut_cells(C, (real)c[0], (real)c[1], (real)c[2]);
    if ((int)q.i < J.nx)
      for (int j = (int)q.j0; j < (int)q.j1 && j < J.ny; j++) {
        const CellRecord& n = J.at((int)q.i, j);
        if (n.is(CT_SOLID)) continue;
        const real w = (C.FT == FT_FLAT) ? C.dy : 2 * M_PI * C.dy * n.y;
        push(LK_M, at((int)q.i, j), at((int)q.i, j), w);
      }
    L.off.push_back(L.nterms());
  }
  return L;
}

// Ring of list values: row s holds the nlists() folds of one step, times[s]
// its time.  -> LoadHistory, oldest first; time_of(t): the reader's clock.
template <class TimeOf>
inline LoadHistory load_history_from_ring(const LoadPlan& L, const real* vals, const double* times, long total, long cap,
                                          TimeOf time_of) {
  LoadHistory H;
  H.nboxes = L.nboxes;
  H.ncuts = L.ncuts;
  H.total = total;
  const size_t nl = (size_t)L.nlists(), nf = (size_t)LOAD_PARTS * L.nboxes;
  std::vector<real> rows;
  ring_oldest_first(vals, nl, times, total, cap, time_of, rows, H.times);
  for (size_t k = 0; k < H.times.size(); k++) {
    const real* row = rows.data() + k * nl;
    H.forces.insert(H.forces.end(), row, row + nf);
    H.mass_flow.insert(H.mass_flow.end(), row + nf, row + nl);
  }
  for (size_t l = 0; l < nl; l++) (l < nf ? H.box_terms : H.cut_terms).push_back(L.off[l + 1] - L.off[l]);
  H.span = L.span;
  return H;
}

}  // namespace hf2d
