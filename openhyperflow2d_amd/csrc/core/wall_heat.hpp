// Per-step wall heat recorder (record_wall_heat): the HeatFlux-X profile (Q,
// Alpha, Cp, St per column) and the HeatFlux-Y profile (Q per row) after every
// sampled step, as heat_flux_x_cols / heat_flux_y_terms + fold_heat_flux_y of
// postproc.cpp give them on a field downloaded after that step.
//
// A node is a CT_WALL_NO_SLIP cell.  Its term reads lam + lam_t of the node
// and of its four neighbours N1..N4 and Tg, p of the node; which node feeds
// which column and row, and in which order, depends only on the flags and the
// neighbour indices: the plan lists that once.  A backend writes (lam + lam_t,
// Tg, p) of every needed cell after a step and folds each list in list order
// with the host's max-or-first rule, so the values are those of the host
// functions bit for bit.  The host functions themselves call the term and fold
// functions below: one expression for the writer, the oracle and both
// recorders.
//
// All expressions are in `real`, in the association written here, one
// operation per statement (nothing to contract).  The divisions are the
// language's `/`: IEEE, correctly rounded on the host and on the device in
// both precisions (a handful of nodes per step: the cost of the full expansion
// does not matter here).
//
// Running statistics per profile entry (4 nx + ny of them), in double in both
// builds, on the sampling decision and the weights of flow_stats.hpp
// (StatsScalars, stats_tick): with the entry's value x, the sample's weight w,
// r = w / W and the sample's time t
//   d = x - m;  m := m + r * d;  e = x - m;  M := M + (w * d) * e
//   first sample: peak = x, peak_time = t;  later: if (x > peak) the same
// var = M / W is formed by the reader.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "case.hpp"
#include "flow_stats.hpp"
#include "ring_history.hpp"

namespace hf2d {

constexpr int WALL_HEAT_X = 4;   // Q, Alpha, Cp, St: the rows of the X profile

// What the terms need besides the cells' values.
struct WallHeatConst {
  real st_den = 1, cp_den = 1, Pg = 0;   // of the Cp flow (wall_heat_consts)
  real Ts0 = 0, dx = 0, dy = 0;
};

// std::max on both sides: a unless a < b
HF_HD inline real wall_heat_max(real a, real b) { return a < b ? b : a; }

// lam_eff of a node from lam + lam_t of the node and of N1..N4, in that order
HF_HD inline real wall_heat_lam_eff(real s0, real s1, real s2, real s3, real s4) {
  real s = s0;
  s += s1;
  s += s2;
  s += s3;
  s += s4;
  return s / (real)5;
}

// q of a node across the spacing d (dy: X profile, dx: Y profile)
HF_HD inline real wall_heat_q(const WallHeatConst& K, real lam_eff, real Tg, real d) {
  const real dT = Tg - K.Ts0;
  const real f = lam_eff * dT;
  return f / d;
}

struct WallHeatXTerm {
  real q, alpha, cp, st;
};
HF_HD inline WallHeatXTerm wall_heat_x_term(const WallHeatConst& K, real lam_eff, real Tg, real p) {
  WallHeatXTerm t;
  t.q = wall_heat_q(K, lam_eff, Tg, K.dy);
  t.alpha = lam_eff / K.dy;
  t.st = t.q / K.st_den;
  const real dp = p - K.Pg;
  t.cp = dp / K.cp_den;
  return t;
}

// The sequential fold: max, or the first value while the old Q is zero.  One
// test on the old Q governs both lines of the X profile.
HF_HD inline void wall_heat_fold_x(real& Q, real& Al, real q, real alpha) {
  if (Q != 0) {
    Q = wall_heat_max(Q, q);
    Al = wall_heat_max(Al, alpha);
  } else {
    Q = q;
    Al = alpha;
  }
}
HF_HD inline void wall_heat_fold_y(real& Q, real q) { Q = Q != 0 ? wall_heat_max(Q, q) : q; }

// One entry's running statistics (see the head of this file).
HF_HD inline void wall_heat_stat(double w, double r, double t, bool first, double x, double& m, double& M,
                                 double& peak, double& peak_time) {
  const double d = x - m;
  const double m1 = m + r * d;
  m = m1;
  const double e = x - m1;
  const double wd = w * d;
  M = M + wd * e;
  if (first || x > peak) {
    peak = x;
    peak_time = t;
  }
}

// st_den, cp_den and Pg of flow `cp_flow` (1-based, Cp_Flow_Index), as
// heat_flux_x_cols and calc_cp form them.  false: no such flow.
inline bool wall_heat_consts(const Case& cs, int cp_flow, WallHeatConst& K) {
  const Config& C = cs.cfg;
  K.Ts0 = C.Ts0;
  K.dx = C.dx;
  K.dy = C.dy;
  if (cp_flow < 1 || cp_flow > (int)cs.flows2d.size()) return false;
  const GasFlow& F = cs.flows2d[cp_flow - 1];
  const real Trec = (1 + 0.45 * (F.kg() - 1.0) * F.flow_MACH() * F.flow_MACH()) * F.Tg();
  K.st_den = F.ROG() * F.Wg2d() * F.C * (Trec - C.Ts0);
  K.cp_den = 0.5 * F.ROG() * F.Wg2d() * F.Wg2d();
  K.Pg = F.Pg();
  return true;
}

// rows [j0, j1) of the X profile for the keys y_min, y_max
inline std::pair<int, int> wall_heat_rows(int y_min, int y_max, int ny) {
  return {std::max(0, y_min), std::min(y_max, ny - 1)};
}

// A ring of sampled rows of `ne` entries with the running statistics of every
// entry, on the host: the CPU backend's recorders keep theirs in one, and a
// device recorder's is read back into one.  The wall heat recorder and the
// surface recorder (surface_plan.hpp) differ only in what an entry is.
struct SampledRing {
  std::vector<real> vals;      // [capacity][ne]
  std::vector<double> times;   // [capacity] time after the sampled step
  std::vector<double> stat;    // m, M, peak, peak_time: [ne] each
  StatsScalars sc;             // the sampling decision and the weights (stats_tick)
  long total = 0;              // samples taken since arming
  // the ring and the statistics restart; the sampling count and the clock (at t_now) with them
  void clear(size_t ne, int every, bool step_weight, double t_now) {
    total = 0;
    sc = StatsScalars{};
    sc.every = every;
    sc.step_weight = step_weight ? 1 : 0;
    sc.t_seen = t_now;
    stat.assign(4 * ne, 0.0);
  }
};

// What both recorders' histories hold: row k of vals is sample k, oldest first.
struct SampledHistory {
  long total = 0;              // samples taken since arming (rows kept: min(total, capacity))
  std::vector<double> times;   // [n] time after the step (the probe recorder's clock)
  std::vector<real> vals;      // [n][ne]
  bool statistics = false;
  std::vector<double> mean, var, peak, peak_time;   // [ne] each
  double time = 0.0;           // W: the weighted time span, or the sample count
  long samples = 0;
};

// Ring and statistics -> history; time_of(t): the reader's clock for a stored time.
template <class TimeOf>
inline void sampled_history_fill(SampledHistory& H, const SampledRing& r, long cap, size_t ne, bool statistics,
                                 TimeOf time_of) {
  H.total = r.total;
  ring_oldest_first(r.vals.data(), ne, r.times.data(), r.total, cap, time_of, H.vals, H.times);
  H.statistics = statistics;
  if (!statistics) return;
  const StatsScalars& sc = r.sc;
  const double* stat = r.stat.data();
  H.time = sc.W;
  H.samples = (long)sc.samples;
  H.mean.assign(stat, stat + ne);
  H.var.assign(stat + ne, stat + 2 * ne);
  H.peak.assign(stat + 2 * ne, stat + 3 * ne);
  H.peak_time.assign(ne, 0.0);
  for (size_t k = 0; k < ne; k++) {
    H.var[k] = sc.samples ? H.var[k] / sc.W : 0.0;
    if (sc.samples) H.peak_time[k] = time_of(stat[3 * ne + k]);
  }
}

// What wall_heat_history() returns: an entry is a profile value, a row
// Q, Alpha, Cp, St [nx] each, then the Y profile [ny].
struct WallHeatHistory : SampledHistory {
  int nx = 0, ny = 0;
  std::vector<long> x_nodes, y_nodes;   // [nx], [ny] nodes of each list (static)
};

struct WallHeatPlan {
  int nx = 0, ny = 0;
  WallHeatConst K;
  std::vector<long> cells;   // unique needed cells (local index): the nodes and their N1..N4
  std::vector<int> node5;    // [nnodes][5] the node and N1..N4 as indices into cells
  std::vector<int> off;      // [nx + ny + 1] first entry of each list: nx columns, then ny rows
  std::vector<int> list;     // the lists' nodes, in the host's order
  int nlists() const { return nx + ny; }
  int nentries() const { return WALL_HEAT_X * nx + ny; }
  long nnodes() const { return (long)node5.size() / 5; }
  long ncells() const { return (long)cells.size(); }
};

// The arming options that the plan is rebuilt from.
struct WallHeatOpts {
  bool x = true, y = true;
  int cp_flow = 0;             // 1-based flow of the X profile
  int y_min = 0, y_max = 0;    // its rows, as the deck's keys
  int every = 1;
  long capacity = 1024;        // 0: statistics only
  bool statistics = true, step_weight = false;
};

inline void check_wall_heat(const WallHeatOpts& o) {
  if (!o.x && !o.y) throw std::invalid_argument("record_wall_heat: neither the X nor the Y profile is requested");
  if (o.every < 1) throw std::invalid_argument("record_wall_heat: every must be at least 1");
  if (o.capacity < 0) throw std::invalid_argument("record_wall_heat: capacity must not be negative");
  if (o.capacity == 0 && !o.statistics)
    throw std::invalid_argument("record_wall_heat: capacity 0 keeps statistics only, and statistics are off");
}

// The plan over the whole field J (one solver, not a strip); local cell of
// global (i, j): (i + l_off) * ny + j.  std::invalid_argument: the X profile
// with a flow index the case does not have.
inline WallHeatPlan build_wall_heat_plan(const Case& cs, const Field& J, const WallHeatOpts& o, int l_off = 0) {
  WallHeatPlan P;
  P.nx = J.nx;
  P.ny = J.ny;
  const bool ok = wall_heat_consts(cs, o.cp_flow, P.K);
  if (o.x && !ok)
    throw std::invalid_argument("record_wall_heat: Cp flow index " + std::to_string(o.cp_flow) + " outside the case's " +
                                std::to_string(cs.flows2d.size()) + " flows");
  if (!ok) P.K.st_den = P.K.cp_den = 1;   // (never read: no column holds a node)
  const auto rows = wall_heat_rows(o.y_min, o.y_max, J.ny);
  std::vector<int> slot((size_t)J.nx * J.ny, -1), node_of((size_t)J.nx * J.ny, -1);
  auto need = [&](int i, int j) {
    int& s = slot[(size_t)i * J.ny + j];
    if (s < 0) {
      s = (int)P.cells.size();
      P.cells.push_back((long)(i + l_off) * J.ny + j);
    }
    return s;
  };
  auto node = [&](int i, int j) {
    int& n = node_of[(size_t)i * J.ny + j];
    if (n < 0) {
      const CellRecord& c = J.at(i, j);
      n = (int)P.nnodes();
      const int q[5][2] = {{i, j}, {i - c.idXl, j}, {i + c.idXr, j}, {i, j + c.idYu}, {i, j - c.idYd}};
      for (const auto& a : q) {
        if (!J.in(a[0], a[1])) throw std::runtime_error("wall heat recorder: a node's neighbour lies outside the grid");
        P.node5.push_back(need(a[0], a[1]));
      }
    }
    return n;
  };
  P.off.push_back(0);
  for (int i = 0; i < J.nx; i++) {   // heat_flux_x_cols
    if (o.x)
      for (int j = rows.first; j < rows.second; j++)
        if (J.at(i, j).is(CT_WALL_NO_SLIP)) P.list.push_back(node(i, j));
    P.off.push_back((int)P.list.size());
  }
  for (int j = 0; j < J.ny; j++) {   // heat_flux_y_terms, folded per row
    if (o.y)
      for (int i = 0; i < J.nx - 1; i++)
        if (J.at(i, j).is(CT_WALL_NO_SLIP)) P.list.push_back(node(i, j));
    P.off.push_back((int)P.list.size());
  }
  return P;
}

// One list folded from the needed cells' values (sl: lam + lam_t, sT: Tg, sp:
// p, indexed like WallHeatPlan::cells): list l < nx is column l and yields
// out[0..3] = Q, Alpha, Cp, St; the others are rows and yield out[0].  An
// empty list is +0.0.
HF_HD inline void wall_heat_list(const WallHeatConst& K, int nx, int l, const int* off, const int* list,
                                 const int* node5, const real* sl, const real* sT, const real* sp, real out[4]) {
  real Q = 0, Al = 0, Cp = 0, St = 0;
  const bool col = l < nx;
  for (int t = off[l]; t < off[l + 1]; t++) {
    const int* c = node5 + 5 * (long)list[t];
    const real lam_eff = wall_heat_lam_eff(sl[c[0]], sl[c[1]], sl[c[2]], sl[c[3]], sl[c[4]]);
    if (col) {
      const WallHeatXTerm x = wall_heat_x_term(K, lam_eff, sT[c[0]], sp[c[0]]);
      wall_heat_fold_x(Q, Al, x.q, x.alpha);
      Cp = x.cp;
      St = x.st;
    } else {
      wall_heat_fold_y(Q, wall_heat_q(K, lam_eff, sT[c[0]], K.dx));
    }
  }
  out[0] = Q;
  out[1] = Al;
  out[2] = Cp;
  out[3] = St;
}

// Position of list l's k-th value in a row of 4 nx + ny entries.
HF_HD inline int wall_heat_entry(int nx, int l, int k) { return l < nx ? k * nx + l : WALL_HEAT_X * nx + (l - nx); }

// Ring and statistics -> WallHeatHistory, oldest first (sampled_history_fill).
template <class TimeOf>
inline WallHeatHistory wall_heat_history_from(const WallHeatPlan& P, const WallHeatOpts& o, const SampledRing& r,
                                              TimeOf time_of) {
  WallHeatHistory H;
  H.nx = P.nx;
  H.ny = P.ny;
  sampled_history_fill(H, r, o.capacity, (size_t)P.nentries(), o.statistics, time_of);
  for (int l = 0; l < P.nlists(); l++) (l < P.nx ? H.x_nodes : H.y_nodes).push_back(P.off[l + 1] - P.off[l]);
  return H;
}

}  // namespace hf2d
