// Plain argument blocks and constants of the lean N-S step (lean_ns.hpp), the
// lean mechanism step (lean_mech.hpp) and the per-step observers (probe, load,
// wall heat, surface and frame recorders; their post-step view and kind dispatch):
// what DeviceSolver::Impl and the host code of every unit need of them, without
// the families' device code.
#pragma once

#include <type_traits>

#include "../core/lean_euler.hpp"
#include "../core/wall_heat.hpp"
#include "../core/surface_plan.hpp"
#include "../core/frame_rule.hpp"

namespace hf2d {

// Kernel argument block.  Level m-1 = the primitives the fill F_m reads
// (prim_old of the split fill), level m = the ones it produces.
struct LnsArrays {
  long N = 0;
  const real* Sp = nullptr;   // Sp^m [k * N + idx] (live equations)
  real* Sp_out = nullptr;     // Sp^{m+1}
  real* beta = nullptr;       // in place
  const real *Ui = nullptr, *Vi = nullptr, *Ti = nullptr;
  real *Uo = nullptr, *Vo = nullptr, *To = nullptr;
  const real *CPi = nullptr, *mui = nullptr, *lami = nullptr, *kki = nullptr, *mu_ti = nullptr;
  real *CPo = nullptr, *muo = nullptr, *lamo = nullptr, *kko = nullptr, *mu_to = nullptr;
  const real *R = nullptr, *BGX = nullptr, *BGY = nullptr, *grad = nullptr, *l_min = nullptr, *y_plus = nullptr;
  // in place (a ring evaluation of another tile discards these outputs, so
  // only the owner's read-before-write matters)
  real* SrcAdd = nullptr;
  real* Src = nullptr;
  // generic fluxes: the turbulence equations' of a node without a k-eps
  // model bit are never rewritten by the fill (constant while lean)
  const real *gA = nullptr, *gB = nullptr, *gF = nullptr;
  const real* dSdx_in = nullptr;
  const real* dSdy_in = nullptr;
  real* dSdx_out = nullptr;
  real* dSdy_out = nullptr;
  const u64* CT = nullptr;
  const u64* TT = nullptr;
  const uint8_t* nb = nullptr;
  const uint8_t* gf = nullptr;
};

constexpr int LNM_NSB = 9;   // species block of the kernel (mechanisms up to 9 species)
constexpr int LNM_TILE = 16;  // tile edge (256 cells, one per thread; the ring is exactly one wavefront)

struct LnmArrays {
  long N = 0;
  const MechData* mech = nullptr;
  int nsp = 0, bath = 0;
  const real* Sp = nullptr;   // Sp^m (flow + turbulence equations, [k * N + idx])
  real* Sp_out = nullptr;     // Sp^{m+1}
  const real* Ys = nullptr;   // species of S^m (after the kinetics), [s * N + idx]
  real* Ys_out = nullptr;     // species of Sp^{m+1} (the kinetics then update them in place)
  real* beta = nullptr;       // in place
  real* betas = nullptr;
  const real *Ui = nullptr, *Vi = nullptr, *Ti = nullptr;   // level m-1 (gradients, velocity recovery)
  real *Uo = nullptr, *Vo = nullptr, *To = nullptr;         // level m
  const real *mui = nullptr, *lami = nullptr, *mu_ti = nullptr;
  real *muo = nullptr, *lamo = nullptr, *mu_to = nullptr;
  const real *Tsi = nullptr, *psi = nullptr, *CPsi = nullptr, *ksi = nullptr;   // state of level m
  real *Tso = nullptr, *pso = nullptr, *CPso = nullptr, *kso = nullptr;         // state of level m+1
  const real *l_min = nullptr, *y_plus = nullptr, *BGX = nullptr, *BGY = nullptr, *grad = nullptr;
  real* Src = nullptr;      // turbulence sources, in place
  real* SrcAdd = nullptr;   // wall sources, in place
  const real *gA = nullptr, *gB = nullptr, *gF = nullptr;   // turbulence fluxes of nodes without the model
  const real* dSdx_in = nullptr;
  const real* dSdy_in = nullptr;
  real* dSdx_out = nullptr;
  real* dSdy_out = nullptr;
  const real* dSdxs_in = nullptr;   // species Cauchy dS (nullptr: no node needs them)
  const real* dSdys_in = nullptr;
  real* dSdxs_out = nullptr;
  real* dSdys_out = nullptr;
  const u64* CT = nullptr;
  const u64* TT = nullptr;
  const uint8_t* nb = nullptr;
  const uint8_t* gf = nullptr;
  int* hot = nullptr;   // reacting cells of the step (kinetics list)
  unsigned* hot_n = nullptr;   // ... and their count (DevScalars::hot_cnt / hot_cnt2 of the slot)
  int part = 0;   // tiles of this launch: 0 all, 1 the strip's edge tile columns, 2 the others (comm overlap)
  unsigned long long* tr = nullptr;   // phase trace (HF2D_LNM_TRACE): 12 clocks per workgroup
  // xGMI mailboxes: the previous step's HALO_LNS list (lg) and the exchange
  // arguments (xg, device copies): the edge tiles copy that step's halo from
  // the mailbox into the ghost columns first (fx_ghost_prologue)
  const struct FusedX* xg = nullptr;
  const struct ColList* lg = nullptr;
};

constexpr int PROBE_MAX = 64;    // one lane per probe
constexpr int PROBE_VARS = 5;    // p, T, rho, U, V
enum { PR_GATHER = 0, PR_SGL = 1, PR_SGT = 2, PR_MECH = 3, PR_LEAN = 4 };

// What every observer's launches read after a step (DeviceSolver::post_step):
// the PR_* kind and the view of the representation that is authoritative now;
// for the lean N-S / mechanism state the views of the fill lns_materialize
// would run (else the same view) and the dt slot that fill reads.
struct PostStep {
  int kind = PR_GATHER;
  SoA s, fin, out;
  int fslot = 0;
};

// The run-time kind as a compile-time constant: f(std::integral_constant<int, PR_*>).
// The one switch over the kinds.  LEAN false: PR_LEAN runs as PR_GATHER and f
// is not instantiated for it (the load recorder has no kernel of that kind).
template <bool LEAN = true, class F>
inline void with_kind(int kind, F&& f) {
  switch (kind) {
    case PR_SGL: return f(std::integral_constant<int, PR_SGL>{});
    case PR_SGT: return f(std::integral_constant<int, PR_SGT>{});
    case PR_MECH: return f(std::integral_constant<int, PR_MECH>{});
    case PR_LEAN:
      if constexpr (LEAN) return f(std::integral_constant<int, PR_LEAN>{});
      [[fallthrough]];
    default: return f(std::integral_constant<int, PR_GATHER>{});
  }
}

struct ProbeRing {
  const long* idx = nullptr;   // local cell of each probe (< 0: another strip's column)
  int n = 0, cap = 0;
  real* rows = nullptr;        // [cap][n][PROBE_VARS]
  double* times = nullptr;     // [cap] DevScalars::time_part after the step
  unsigned long long* count = nullptr;   // rows written since arming
};

// Per-step load recorder (load_history.hpp): the plan, one entry per term, and the ring
struct LoadsDev {
  // the plan (LoadPlan), one entry per term
  const long* cell = nullptr;
  const long* cell2 = nullptr;
  const real* coef = nullptr;
  const uint8_t* kind = nullptr;
  const long* off = nullptr;   // [nlists + 1]
  long nterms = 0;
  int nlists = 0, cap = 0;
  real* scratch = nullptr;     // [nterms] the step's term values
  real* vals = nullptr;        // [cap][nlists]
  double* times = nullptr;     // [cap] DevScalars::time_part after the step
  unsigned long long* count = nullptr;   // rows written since arming
};

// Per-step wall heat recorder (wall_heat.hpp): what its tick leaves for the
// two kernels behind it, the plan, the ring and the statistics
struct WallHeatScalars {
  StatsScalars s;   // the sampling decision and the weights (stats_tick)
  long slot = 0;    // ring row of this sample
};
// The ring of sampled rows and the running statistics of a recorder that ticks
// on scalars of its own: `ne` entries a row (wall heat: 4 nx + ny; surface:
// [SURFACE_NVARS][nnodes])
struct SampleRing {
  real* vals = nullptr;          // [cap][ne]
  double* times = nullptr;       // [cap] DevScalars::time_part after the step
  double* stat = nullptr;        // [4][ne] m, M, peak, peak_time (DevScalars::time_part)
  WallHeatScalars* sc = nullptr;
  int cap = 0, statistics = 0;
};
struct WallHeatDev {
  WallHeatConst K;
  // the plan (WallHeatPlan)
  const long* cells = nullptr;   // [ncells]
  const int* node5 = nullptr;    // [nnodes][5]
  const int* off = nullptr;      // [nx + ny + 1]
  const int* list = nullptr;
  long ncells = 0;
  int nx = 0, ny = 0;
  real* scratch = nullptr;       // [3][ncells] lam + lam_t, Tg, p of the needed cells after the step
  SampleRing ring;
};

// Per-step surface recorder (surface_history.hpp): the plan, the ring and the
// statistics; the tick's scalars are the wall heat recorder's kind, its own
struct SurfaceDev {
  WallHeatConst K;
  // the plan (SurfacePlan)
  const long* cells = nullptr;     // [ncells]
  const uint8_t* mask = nullptr;   // [ncells] SurfaceCellBit
  const int* idx = nullptr;        // [nnodes][SURFACE_IDX]
  const uint8_t* bits = nullptr;   // [nnodes] SurfaceNodeBit
  long ncells = 0, nnodes = 0;
  real* scratch = nullptr;         // [SURFACE_PLANES][ncells] the needed cells' values after the step
  SampleRing ring;
};

// Per-step frame recorder (frame_history.hpp): the geometry, the rows of its
// box and the ring (no statistics); the tick's scalars are the wall heat
// recorder's kind, its own
struct FrameDev {
  FrameGeom G;
  real* scratch = nullptr;         // [FRAME_ROW][G.nbox()] the rows of the box's gas cells after the step
  SampleRing ring;                 // vals: [cap][nvars][ni][nj]
};

}  // namespace hf2d
