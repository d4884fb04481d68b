// Field frames (record_frames, Case.frame): the probe recorder's row
// (p, T, rho, U, V) of every cell of a strided region, and five variables
// formed from the rows of the cell and its four neighbours -- the density and
// the pressure gradient magnitude (numerical schlieren), the vorticity, the
// dilatation and the Ducros sensor.  One rule, frame_cell, which the device
// kernel (hip/frame_history.hpp), the CPU backend and the host oracle call.
//
// A cell is gas when its CT has CT_NODE_IS_SET and not CT_SOLID.  For a gas
// cell (i, j) of the nx x ny grid, in `real`, in exactly this association and
// without contraction:
//   hasW = i > 0 && gas(i-1, j), hasE = i+1 < nx && gas(i+1, j); hasS / hasN in j
//   ix = (1 / dx) / max(hasW + hasE, 1), iy = (1 / dy) / max(hasS + hasN, 1)
//   ddx(q) = (q_E - q_W) * ix, a missing neighbour replaced by the cell's own
//            value: central with both, one-sided with one, +0 with none; ddy in j
//   grad_rho   = sqrt(ddx(rho) ddx(rho) + ddy(rho) ddy(rho)); grad_p likewise
//   vorticity  = ddx(V) - ddy(U)
//   dilatation = ddx(U) + ddy(V)
//   ducros     = th th / ((th th + om om) + 1e-30), th the dilatation, om the vorticity
// The divisions are plain `/` and the root is the correctly rounded one (not
// hf_div / hf_sqrt, whose exactness excludes the exponent limits a squared
// gradient can reach).  A non-gas cell reads +0.0 in every variable.  The planar
// expressions are used on axisymmetric decks too: there is no V / y term.
#pragma once

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "common.hpp"

namespace hf2d {

constexpr int FRAME_NVARS = 10;
constexpr int FRAME_ROW = 5;   // the probe recorder's row: p, T, rho, U, V
enum FrameVar { FV_P = 0, FV_T, FV_RHO, FV_U, FV_V, FV_GRAD_RHO, FV_GRAD_P, FV_VORTICITY, FV_DILATATION, FV_DUCROS };
constexpr unsigned FRAME_GRAD_MASK = ((1u << FRAME_NVARS) - 1u) & ~((1u << FRAME_ROW) - 1u);   // the stencil variables
inline const char* const* frame_var_names() {
  static const char* const n[FRAME_NVARS] = {"p", "T", "rho", "U", "V", "grad_rho", "grad_p", "vorticity", "dilatation",
                                             "ducros"};
  return n;
}

enum FrameNb { FN_C = 0, FN_W, FN_E, FN_S, FN_N };

HF_HD inline bool frame_gas(u64 ct) { return has_all(ct, CT_NODE_IS_SET) && !has_all(ct, CT_SOLID); }

// The armed variables of one gas cell into out[v] (v: FrameVar; what the mask
// does not ask for is left alone).  q(nb, v): variable v of the row of the
// cell (FN_C) or of a neighbour, which is asked for only where has* says so.
template <class Q>
HF_HD inline void frame_cell(unsigned mask, bool hasW, bool hasE, bool hasS, bool hasN, real dx, real dy, const Q& q,
                             real out[FRAME_NVARS]) {
#pragma unroll
  for (int v = 0; v < FRAME_ROW; v++)
    if (mask & (1u << v)) out[v] = q(FN_C, v);
  if (!(mask & FRAME_GRAD_MASK)) return;
  const int nxn = (hasW ? 1 : 0) + (hasE ? 1 : 0), nyn = (hasS ? 1 : 0) + (hasN ? 1 : 0);
  const real mx = (real)(nxn > 1 ? nxn : 1), my = (real)(nyn > 1 ? nyn : 1);
  const real ix = ((real)1.0 / dx) / mx;
  const real iy = ((real)1.0 / dy) / my;
  auto ddx = [&](int v) {
    const real c = q(FN_C, v);
    const real e = hasE ? q(FN_E, v) : c, w = hasW ? q(FN_W, v) : c;
    return (e - w) * ix;
  };
  auto ddy = [&](int v) {
    const real c = q(FN_C, v);
    const real n = hasN ? q(FN_N, v) : c, s = hasS ? q(FN_S, v) : c;
    return (n - s) * iy;
  };
  if (mask & (1u << FV_GRAD_RHO)) {
    const real gx = ddx(FV_RHO), gy = ddy(FV_RHO);
    const real a = gx * gx, b = gy * gy;
    out[FV_GRAD_RHO] = std::sqrt(a + b);
  }
  if (mask & (1u << FV_GRAD_P)) {
    const real gx = ddx(FV_P), gy = ddy(FV_P);
    const real a = gx * gx, b = gy * gy;
    out[FV_GRAD_P] = std::sqrt(a + b);
  }
  if (mask & ((1u << FV_VORTICITY) | (1u << FV_DILATATION) | (1u << FV_DUCROS))) {
    const real om = ddx(FV_V) - ddy(FV_U);
    const real th = ddx(FV_U) + ddy(FV_V);
    if (mask & (1u << FV_VORTICITY)) out[FV_VORTICITY] = om;
    if (mask & (1u << FV_DILATATION)) out[FV_DILATATION] = th;
    if (mask & (1u << FV_DUCROS)) {
      const real t2 = th * th, o2 = om * om;
      out[FV_DUCROS] = t2 / ((t2 + o2) + (real)1e-30);
    }
  }
}

// What a recorder is armed with / Case.frame is asked for.
struct FrameOpts {
  std::vector<std::string> vars;   // names of frame_var_names(), none twice
  bool whole = true;               // region: the whole grid
  int i0 = 0, i1 = 0, j0 = 0, j1 = 0;   // else [i0, i1) x [j0, j1)
  int si = 1, sj = 1;
  int every = 1;
  long capacity = 16;
};

// The output cells i0 + a si (a < ni), j0 + b sj (b < nj) of the nx x ny grid,
// the armed variables, and the box [di0, di1) x [dj0, dj1) of cells whose rows
// the rule reads: the output cells' span, with a stencil variable armed dilated
// by one cell and clipped to the grid.  Plain data: a kernel argument.
struct FrameGeom {
  int nx = 0, ny = 0;
  int i0 = 0, j0 = 0, si = 1, sj = 1, ni = 0, nj = 0;
  int di0 = 0, di1 = 0, dj0 = 0, dj1 = 0;
  int ioff = 0;   // local column of global column i in the backend's arrays: i + ioff
  int nvars = 0;
  int var[FRAME_NVARS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // FrameVar of each output plane
  unsigned mask = 0;
  real dx = 1, dy = 1;
  HF_HD long ncells() const { return (long)ni * nj; }
  HF_HD long nbox() const { return (long)(di1 - di0) * (dj1 - dj0); }
  HF_HD long box_at(int i, int j) const { return (long)(i - di0) * (dj1 - dj0) + (j - dj0); }
};

// std::invalid_argument: an unknown, repeated or empty vars, a region that is
// empty or outside the grid, a stride below 1, every < 1, capacity < 1, a ring
// of more than 2^31 entries.  [own0, own1): the global columns the caller
// holds (a strip keeps the output columns it owns; the whole grid otherwise).
inline FrameGeom frame_geom(const std::string& who, const FrameOpts& o, int nx, int ny, real dx, real dy, int own0,
                            int own1, int ioff) {
  FrameGeom G;
  G.nx = nx;
  G.ny = ny;
  G.dx = dx;
  G.dy = dy;
  G.ioff = ioff;
  if (o.vars.empty()) throw std::invalid_argument(who + ": no variables");
  for (const std::string& name : o.vars) {
    int v = -1;
    for (int k = 0; k < FRAME_NVARS; k++)
      if (name == frame_var_names()[k]) v = k;
    if (v < 0) {
      std::string all;
      for (int k = 0; k < FRAME_NVARS; k++) all += std::string(k ? ", " : "") + frame_var_names()[k];
      throw std::invalid_argument(who + ": unknown variable '" + name + "' (one of " + all + ")");
    }
    if (G.mask & (1u << v)) throw std::invalid_argument(who + ": variable '" + name + "' is listed twice");
    G.mask |= 1u << v;
    G.var[G.nvars++] = v;
  }
  const int i0 = o.whole ? 0 : o.i0, i1 = o.whole ? nx : o.i1, j0 = o.whole ? 0 : o.j0, j1 = o.whole ? ny : o.j1;
  if (i0 < 0 || j0 < 0 || i1 > nx || j1 > ny)
    throw std::invalid_argument(who + ": the region [" + std::to_string(i0) + ", " + std::to_string(i1) + ") x [" +
                                std::to_string(j0) + ", " + std::to_string(j1) + ") lies outside the " +
                                std::to_string(nx) + " x " + std::to_string(ny) + " grid");
  if (i0 >= i1 || j0 >= j1) throw std::invalid_argument(who + ": the region is empty");
  if (o.si < 1 || o.sj < 1) throw std::invalid_argument(who + ": a stride must be at least 1");
  if (o.every < 1) throw std::invalid_argument(who + ": every must be at least 1");
  if (o.capacity < 1) throw std::invalid_argument(who + ": capacity must be at least 1");
  G.si = o.si;
  G.sj = o.sj;
  // the output columns the caller owns: a = a0 .. a1 - 1 of i0 + a si
  const long a_all = (i1 - i0 + o.si - 1) / o.si;
  long a0 = own0 > i0 ? ((long)(own0 - i0) + o.si - 1) / o.si : 0;
  long a1 = own1 < i1 ? (own1 > i0 ? ((long)(own1 - i0) + o.si - 1) / o.si : 0) : a_all;
  if (a0 > a_all) a0 = a_all;
  if (a1 < a0) a1 = a0;
  G.i0 = i0 + (int)a0 * o.si;
  G.ni = (int)(a1 - a0);
  G.j0 = j0;
  G.nj = (j1 - j0 + o.sj - 1) / o.sj;
  const double ring = (double)o.capacity * (double)G.nvars * (double)G.ni * (double)G.nj;
  if (ring > 2147483648.0)
    throw std::invalid_argument(who + ": a ring of " + std::to_string(o.capacity) + " x " + std::to_string(G.nvars) +
                                " x " + std::to_string(G.ni) + " x " + std::to_string(G.nj) + " entries, at most 2^31");
  const int d = (G.mask & FRAME_GRAD_MASK) ? 1 : 0;
  if (G.ni > 0) {
    G.di0 = std::max(G.i0 - d, 0);
    G.di1 = std::min(G.i0 + (G.ni - 1) * G.si + 1 + d, nx);
    G.dj0 = std::max(G.j0 - d, 0);
    G.dj1 = std::min(G.j0 + (G.nj - 1) * G.sj + 1 + d, ny);
  }
  return G;
}

// One output cell (a, b) of the geometry into out[v] (v: FrameVar; every
// variable +0.0 for a non-gas cell).  gas(i, j), row(i, j, v): the flags and
// the rows of the global cell (i, j), asked only inside the grid.
template <class Gas, class Row>
inline void frame_eval_cell(const FrameGeom& G, int a, int b, const Gas& gas, const Row& row, real out[FRAME_NVARS]) {
  for (int v = 0; v < FRAME_NVARS; v++) out[v] = 0.0;
  const int i = G.i0 + a * G.si, j = G.j0 + b * G.sj;
  if (!gas(i, j)) return;
  const bool st = (G.mask & FRAME_GRAD_MASK) != 0;
  const bool hasW = st && i > 0 && gas(i - 1, j), hasE = st && i + 1 < G.nx && gas(i + 1, j);
  const bool hasS = st && j > 0 && gas(i, j - 1), hasN = st && j + 1 < G.ny && gas(i, j + 1);
  auto q = [&](int nb, int v) {
    return row(i + (nb == FN_E) - (nb == FN_W), j + (nb == FN_N) - (nb == FN_S), v);
  };
  frame_cell(G.mask, hasW, hasE, hasS, hasN, G.dx, G.dy, q, out);
}

// Every output cell: vals [nvars][ni][nj].
template <class Gas, class Row>
inline void frame_eval(const FrameGeom& G, const Gas& gas, const Row& row, real* vals) {
  const long nc = G.ncells();
  for (int a = 0; a < G.ni; a++)
    for (int b = 0; b < G.nj; b++) {
      real out[FRAME_NVARS];
      frame_eval_cell(G, a, b, gas, row, out);
      for (int k = 0; k < G.nvars; k++) vals[(long)k * nc + (long)a * G.nj + b] = out[G.var[k]];
    }
}

// What frame_history() returns: row k of vals is sample k, oldest first.
struct FrameHistory {
  FrameGeom G;
  long total = 0;              // samples taken since arming (rows kept: min(total, capacity))
  std::vector<double> times;   // [n] time after the step (the probe recorder's clock)
  std::vector<real> vals;      // [n][nvars][ni][nj]
  std::vector<uint8_t> gas;    // [ni][nj]
};

}  // namespace hf2d
