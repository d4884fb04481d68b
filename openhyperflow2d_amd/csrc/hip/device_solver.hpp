// DeviceSolver: MI355X backend of the DEEPS time march (see device_solver.hip).
#pragma once

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../core/solver.hpp"
#include "device_knobs.hpp"

namespace hf2d {

struct LnmArrays;
struct LeanTile;
struct PostStep;

bool gpu_available();
// Largest number of slots per thread that the single-gas lean tile kernel of
// nt threads and cpt cells per thread stages in one batch (lean_tile.hpp); a
// tile that needs more runs the staging loop.  0: no such kernel.
int lean_tile_stage_kmax(int nt, int cpt);
// Cp_air at up to 64 values xv for the table (x, y), evaluated on the device
// the way the single-gas lean tile kernels do (AirTable built by
// air_table_build, staged into LDS, air_table_eval; table_eval on the pack
// for a table in mode 0); returns the values and the mode.
std::pair<std::vector<double>, int> air_table_probe(const std::vector<double>& x, const std::vector<double>& y,
                                                    const std::vector<double>& xv);

// In-process stand-in for the RCCL communicator: N DeviceSolvers (one host
// thread each, possibly sharing one GPU) exchange halo buffers with D2D
// copies and reduce scalars on the host.  Same call sites and pack layout as
// the RCCL path; lets the strip decomposition be verified on a single GPU
// (RCCL refuses two ranks on one device).
struct LocalGroup {
  explicit LocalGroup(int n_)
      : n(n_), send_l(n_), send_r(n_), dt_src(n_, nullptr), vals(n_), packs(n_), blobs(n_) {
    const char* j = std::getenv("HF2D_LOCAL_JITTER_US");
    jitter_us = j ? std::max(0, std::atoi(j)) : 0;
  }
  int n;
  std::mutex mu;
  std::condition_variable cv;
  int arrived = 0;
  long gen = 0;
  // race probe (HF2D_LOCAL_JITTER_US = J > 0): every rank sleeps a
  // pseudo-random 0..J us before each barrier, so the threads reach the
  // collectives and the D2D halo copies in varying orders; a result that
  // depends on that order is an ordering hole (tools/strip_outputs_check.py)
  int jitter_us = 0;
  unsigned long long jitter_state = 0x9E3779B97F4A7C15ull;
  void jitter() {
    unsigned long long x;
    {
      std::lock_guard<std::mutex> lk(mu);
      jitter_state ^= jitter_state << 13;
      jitter_state ^= jitter_state >> 7;
      jitter_state ^= jitter_state << 17;
      x = jitter_state;
    }
    std::this_thread::sleep_for(std::chrono::microseconds((long)(x % (unsigned long long)jitter_us)));
  }
  std::vector<real*> send_l, send_r;
  std::vector<const unsigned long long*> dt_src;   // device dt slot of each rank
  std::vector<double> vals;
  std::vector<ResidualPack> packs;
  std::vector<std::string> blobs;   // allgather_bytes slots
  void barrier() {
    if (jitter_us > 0) jitter();
    std::unique_lock<std::mutex> lk(mu);
    const long g = gen;
    if (++arrived == n) {
      arrived = 0;
      gen++;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
  }
  double reduce(int rank, double v, int op) {   // 0 min, 1 sum, 2 max
    vals[rank] = v;
    barrier();
    double r = vals[0];
    for (int q = 1; q < n; q++) r = op == 0 ? std::min(r, vals[q]) : op == 1 ? r + vals[q] : std::max(r, vals[q]);
    barrier();
    return r;
  }
};

std::shared_ptr<LocalGroup> make_local_group(int n);

// The tuning knobs (split_xcd, lean_cpt, tile_stagger, ...) are the members of
// DeviceKnobs: one row each in device_knobs.hpp.
class DeviceSolver : public SolverBase, public DeviceKnobs {
 public:
  DeviceSolver(Case& cs, int device = 0, int gi0 = 0, int gi1 = -1);
  ~DeviceSolver() override;
  StepResult do_step(const StepParams& P, bool want_res) override;
  StepResult do_step_eager(const StepParams& P, bool want_res);
  std::pair<int, int> owned_columns() const override { return {gi0, gi1}; }
  void download(Field& J) override;
  void upload() override;
  void cycle_update() override;
  void sync_scalars() override;
  void on_cycle_roll() override;
  void poison_cell(int gi, int j) override;
  void sample_monitors(std::vector<MonitorPoint>& mp) override;
  // per-step recorder (hip/probe_history.hpp): hf2d_probe_record is the last
  // launch of every step while armed; reading the history neither leaves the
  // lean state nor changes a ping-pong parity
  void record_probes(const std::vector<std::pair<int, int>>& cells, long capacity) override;
  ProbeHistory probe_history() override;
  void clear_probe_history() override;
  // whole-field statistics (hip/flow_stats.hpp): hf2d_stats_tick and
  // hf2d_stats_accum follow the recorder's launch while armed; reading the
  // averages neither leaves the lean state nor changes a ping-pong parity
  // (with favre or species armed hf2d_stats_accum_x takes the cell pass)
  void start_averaging(int every, bool second_moments, bool step_weight, bool favre = false,
                       const std::vector<int>& species = {}) override;
  void reset_averaging() override;
  void stop_averaging() override;
  FlowAverages averages() override;
  // per-step load recorder (hip/load_history.hpp): hf2d_loads_terms and
  // hf2d_loads_fold follow the step while armed; reading the history neither
  // leaves the lean state nor changes a ping-pong parity
  void record_loads(const std::vector<LoadBox>& boxes, const std::vector<LoadCut>& cuts, long capacity) override;
  LoadHistory load_history() override;
  void clear_load_history() override;
  // per-step wall heat recorder (hip/wall_heat.hpp): hf2d_wallq_tick,
  // hf2d_wallq_cells and hf2d_wallq_fold follow the step while armed; reading
  // the history neither leaves the lean state nor changes a ping-pong parity
  void record_wall_heat(const WallHeatOpts& o) override;
  WallHeatHistory wall_heat_history() override;
  void clear_wall_heat() override;
  // per-step surface recorder (hip/surface_history.hpp): hf2d_wallq_tick,
  // hf2d_surf_cells and hf2d_surf_nodes follow the step while armed; reading
  // the history neither leaves the lean state nor changes a ping-pong parity
  void record_surface(const SurfaceOpts& o) override;
  SurfaceHistory surface_history() override;
  const SurfacePlan& surface_plan() const override;
  void clear_surface() override;
  // per-step frame recorder (hip/frame_history.hpp): hf2d_wallq_tick,
  // hf2d_frame_rows and hf2d_frame_store follow the step while armed; reading
  // the history neither leaves the lean state nor changes a ping-pong parity
  void record_frames(const FrameOpts& o) override;
  FrameHistory frame_history() override;
  void clear_frames() override;
  void trace_push(const char* name) override;
  void trace_pop() override;
  // the eligibility results, step counters, last tile launch and halo
  // transport below, as the Python attributes of the same names give them
  // (sk_mode: what the case is eligible for; split_mode: what the knobs let
  // the split stepper run)
  std::string profile_path_facts() const override;
  const char* halo_transport() const;   // "none" (one rank), "p2p", "local" or "rccl"
  void synchronize();
  // ThreadBlockSize = 0: time the lean tile geometries, keep the fastest (before the first step)
  std::string autotune(int steps = 120);
  std::vector<unsigned long long> trace_tile(int steps = 20);
  void* stream() const;

  // Multi-GPU: RCCL communicator over the strip ranks.
  static std::string nccl_unique_id();
  void init_comm(const std::string& uid, int rank, int nranks);
  // in-process virtual ranks (tests on one GPU; see LocalGroup)
  void init_local(std::shared_ptr<LocalGroup> g, int rank);
  // Multi-GPU: xGMI peer-to-peer mailboxes (hf2d_p2p_xchg).  Every rank
  // exports a descriptor, the descriptors are all-gathered by the caller
  // (torch.distributed, any backend) and imported on every rank; from then on
  // the per-step halo + dt exchange is one device kernel (no RCCL, no host).
  std::string p2p_export(int rank, int nranks);
  void p2p_import(const std::vector<std::string>& descs);
  // timing stand-in: rank `rank` of `nranks` with every peer ready and the
  // neighbours' mailboxes looped back into this rank's own (device_solver.hip)
  void p2p_loopback(int rank, int nranks);
  bool p2p_active() const;
  const struct ColList* lc_device(const struct ColList& L);
  void p2p_complete(bool keep_lns = false);
  struct FusedX fused_args() const;
  const struct FusedX* fx_device(const struct FusedX& X);
  void p2p_set(bool on);   // off: fall back to RCCL/local; on: only after p2p_import
  int comm_rank() const;
  int comm_size() const;
  void exchange(int group, int dt_slot = -1, void* on_stream = nullptr, bool full = false);
  void exchange_dt(int dt_slot);
  int split_mode() const; // SK_* mode of the split stepper (step_split)
  // device columns of the fields a halo group carries, in pack order
  void halo_fields(int group, std::vector<real*>& f, bool full = false) const;
  // (o: column offset of each entry, 1 = the second column of a two-column halo)
  void halo_fields(int group, std::vector<real*>& f, std::vector<unsigned char>& o, bool full) const;
  // p2p self-validation (collective over the strip ranks, before the first
  // step): poisons the ghost columns, runs one mailbox exchange of the full
  // state group with a rank-tagged dt, restores the device scalars and
  // returns this rank's checksums of the columns it sent and received and of
  // the folded dt.  p2p_probe_ok checks the all-gathered blobs of every rank.
  std::string p2p_probe();
  std::vector<unsigned long long> fx_trace();   // fused-exchange tail phase clocks (fx_skip bit 4)
  static bool p2p_probe_ok(const std::vector<std::string>& blobs, int rank, std::string* why);
  void p2p_fallback();   // p2p off, ghost columns refilled over RCCL / the local group

  std::vector<unsigned long long> lnm_trace_fetch();   // lnm_trace: 12 clocks / ids per workgroup
  void set_lean_plain(bool on);   // (re-uploads the flag bytes: lean_plain has no plain setter)
  void lean_materialize();
  void lns_materialize();
  void flush_pending();

  // ---- results: what construction / upload found eligible, what the last step ran ----
  bool lean_ok = false;
  std::string lean_why;
  bool lean_sg_ok = false;
  bool lean_has_cauchy_x = true;   // some node reads dS/dx of an x neighbour (halo must carry it)
  bool any_cauchy_x = true;   // some node applies d2/dx2 = 0 (reads dS/dx of an x neighbour)
  bool sgl_ok = false;
  std::string sgl_why;
  int sk_mode = 0;        // SK_GENERIC / SK_SGL / SK_SGT (stepkern.hpp)
  bool lns_ok = false;    // flat, SK_SGL, adiabatic walls, no sources; one strip
  std::string lns_why;
  int lns_turb = 2;       // turbulence set of the SGT kernel: 2 k-eps, 3 SST, 4 Spalart-Allmaras
  bool lnm_ok = false;
  std::string lnm_why;
  int lnm_turb = 0;       // fill_node turbulence set of the kernel: 0 none, 3 SST
  bool chem_fast_ok = false;   // the loaded mechanism equals a compiled one
  bool chem_rtc_ok = false;
  std::string chem_rtc_why;
  std::string chem_kernel_used;
  // geometry and variant of the last lean tile launch do_step issued (a step
  // on any other kernel clears it: nt == 0); stagger: the start delay the
  // launched kernel applies (0 where it is compiled out), var: 0 plain,
  // 1 outputs, 2 residual; seen: bit v set for every variant v launched in
  // the unbroken run of tile steps with this nt and cpt that the last one
  // ends (the last step of a host call is never a plain one); dt_read: how
  // it read the step's dt (StepParams::dt_read); stage: slots per thread of
  // the batched staging, 0 for the staging loop (LeanTile::stage); table: 1
  // where it evaluated Cp_air from the AirTable in LDS, 0 where it ran
  // table_eval on the species pack (LeanTile::table).  Tests assert through
  // it which variant ran.
  struct TileLast {
    int nt = 0, cpt = 0, TI = 0, TJ = 0, nbi = 0, nbj = 0, stagger = 0, fx = 0, var = 0, seen = 0, dt_read = 0;
    int stage = 0, table = 0;
  };
  TileLast lean_tile_last;
  int air_table_mode = 0;   // AirTable::mode of the uploaded species pack

  // ---- counters ----
  long nstep = 0;
  long lns_steps = 0, lnm_steps = 0;
  long lns_fx_steps = 0;    // lean N-S steps with the fused xGMI mailbox exchange
  long lns_prologue_steps = 0;   // fused lean N-S steps that unpacked the previous halo themselves
  long p2p_mwg_exchanges = 0;   // mailbox exchanges through hf2d_p2p_push / hf2d_p2p_unpack
  long overlap_steps = 0;
  long graph_launches = 0;
  long graph_captures = 0;   // windows captured (a replay needs the same mode_signature)
  // lnm_timing: per-phase device time of the lean mechanism step (tile kernel,
  // kinetics, reacting-cell state kernel; ms summed) and the launches timed ([3])
  double lnm_phase_ms[4] = {0, 0, 0, 0};

  // ---- state ----
  HostArrays h;           // host staging copy
  int dev = 0;
  int gi0 = 0, gi1 = 0, l_off = 0;
  int abuf = 0, dsbuf = 0, pbuf = 0, sbuf = 0;  // ping-pong indices (sbuf: current state)
  // a lean step's output arrays become the state (the split and fused Euler
  // steps flip other subsets and write theirs out)
  void flip_state() {
    sbuf = 1 - sbuf;
    dsbuf = 1 - dsbuf;
    pbuf = 1 - pbuf;
  }
  int cbuf = 0;           // lean N-S: CP/mu/lam/k level ping-pong (0: the generic arrays)
  int lean_state = 0;     // 1: lean arrays authoritative (A/B/F/p stale)
  int lns_state = 0;      // 1: lean N-S buffers authoritative (committed S, A/B/F, p stale); shared with the lean mechanism path
  bool lean_plain = false; // flag-free predictor fast path (measured slower: off; set_lean_plain)
  bool lean_T_stored = true;    // the last lean inviscid step stored T (every kernel but the plain tile variant)
  int lns_prev_mu_t = -1;  // is_mu_t of the previous step (the split fill F_m ran with it)
  double time_offset = 0.0, last_dev_time = 0.0;
  bool dt_word_valid = false;
  unsigned long long* tile_trace = nullptr;   // set only inside trace_tile
  std::vector<long> probe_idx_host;
  std::vector<real> probe_buf_host;
  // The six observers.  Armed: the plan and the arrays exist.  A cached graph
  // window bakes an observer's launches and arrays in, so arming, re-arming,
  // stopping or a plan rebuilt by upload() bumps observers_gen
  // (mode_signature: no window captured before replays after).  autotune()'s
  // trial steps are not the run's: while observers_paused, an armed observer
  // sits them out -- no launch, and nothing the step does for a recorder.
  int observers_gen = 0;
  bool observers_paused = false;
  long probe_cap = 0;           // 0: not armed
  std::vector<long> probe_rec_idx;   // local cell of each probe (-1: another strip's column)
  bool stats_on = false;        // the two kernels are launched
  bool stats_armed = false;     // planes exist (on, or stopped: averages() reads the frozen result)
  bool stats_second = false;
  bool stats_favre = false;
  std::vector<int> stats_species;   // mechanism indices of the listed species
  long loads_cap = 0;           // 0: not armed
  bool loads_friction = false;  // the armed plan holds friction terms: the split fills store their gradients every step
  LoadPlan loads_plan;          // host copy of the armed plan
  std::vector<LoadBox> loads_boxes;
  std::vector<LoadCut> loads_cuts;
  bool wallq_armed = false;
  WallHeatOpts wallq_opts;      // what the plan is rebuilt from
  WallHeatPlan wallq_plan;      // host copy of the armed plan
  bool surf_armed = false;
  bool surf_friction = false;   // the armed plan holds friction terms (as loads_friction)
  SurfaceOpts surf_opts;        // what the plan is rebuilt from
  SurfacePlan surf_plan;        // host copy of the armed plan
  bool frames_armed = false;
  FrameOpts frames_opts;        // what the recorder was armed with (capacity: the ring's)
  // armed and not paused: the step launches the observer
  bool probes_live() const { return probe_cap > 0 && !observers_paused; }
  bool stats_live() const { return stats_on && !observers_paused; }
  bool loads_live() const { return loads_cap > 0 && !observers_paused; }
  bool wallq_live() const { return wallq_armed && !observers_paused; }
  bool surf_live() const { return surf_armed && !observers_paused; }
  bool frames_live() const { return frames_armed && !observers_paused; }
  // the split fills store their gradients every step while a recorder reads them
  bool friction_recorded() const { return (loads_live() && loads_friction) || (surf_live() && surf_friction); }
  bool fx_pending = false;   // fused tile steps left the newest ghost columns and dt in the mailbox (p2p_complete)
  // fused lean N-S steps: the last step's halo is still in the mailbox; the
  // next fused step's edge tiles unpack it (lns_ghost_prologue)
  bool lns_ghost_pending = false, lns_last_valid = false, lns_prev_valid = false;
  int lns_pro_uses = 0;
  int ghost_mode = -1;    // SK_* mode the ghost columns were last exchanged for (-1: complete)
  bool ghost_stale = false;   // the ghost columns hold another stepper's representation (refresh before a split step)
  std::vector<uint8_t> lean_bytes;
  ScenarioTables scen_host;   // staged for upload (must outlive the async copy)
  std::unique_ptr<Comm> host_comm;

 private:
  struct Impl;
  std::unique_ptr<Impl> impl;
  struct GraphCache;
  std::unique_ptr<GraphCache> graph;
  std::vector<StepParams> pending;
  void run_graph();
  // The observers' launches at the end of do_step_eager, in this order, each
  // over the one PostStep of the step; nothing in them allocates, copies or
  // synchronises.
  PostStep post_step(int slot, int slot_next) const;
  void launch_probe_record(const StepParams& P, const PostStep& v);
  void launch_stats(const StepParams& P, const PostStep& v);
  void launch_loads(const StepParams& P, const PostStep& v);       // the load recorder's two launches
  void launch_wall_heat(const StepParams& P, const PostStep& v);   // the wall heat recorder's three launches
  void launch_surface(const StepParams& P, const PostStep& v);     // the surface recorder's three launches
  void launch_frames(const StepParams& P, const PostStep& v);      // the frame recorder's three launches
  void lns_fill_views(SoA& sin, SoA& out) const;   // the views lns_materialize's fill would run over now
  int post_step_view(SoA& s) const;                // PR_* kind and view of the post-step buffers
  // A recorder's plan over the records the backend holds now (throws where a
  // value could not be recorded exactly), and a built plan into the device arrays.
  LoadPlan loads_plan_build(const std::vector<LoadBox>& boxes, const std::vector<LoadCut>& cuts) const;
  void loads_plan_upload(LoadPlan&& P);
  WallHeatPlan wallq_plan_build(const WallHeatOpts& o) const;
  void wallq_plan_upload(WallHeatPlan&& P);
  SurfacePlan surf_plan_build(const SurfaceOpts& o) const;
  void surf_plan_upload(SurfacePlan&& P);
  void refuse_wall_nodes(const std::string& who, const char* nodes, bool wall_T) const;   // the two rules that refuse such a plan
  void plans_rebuild();                   // upload() replaced the records under the armed recorders
  double host_time(double t_dev) const;   // the host's time of a stored DevScalars::time_part
  std::vector<StatsScalars*> tick_scalars() const;   // device scalars of every armed tick: accumulator, wall heat, surface, frames
  uint64_t mode_signature() const;   // kernel-selecting state (graph windows replay only under the same)
  // One step (do_step_eager): the kernels that run it, what every path reads
  // of the step, and what a path reports to the common tail.
  enum class StepPath { Tile, LeanFlat, FusedEuler, LeanMech, LeanNs, Split };
  struct StepCtx {
    StepParams P;          // completed for this strip
    bool want_res;
    int slot, slot_next, serial;
    unsigned nblk;         // workgroups of a one-cell-per-thread launch over the owned cells [c0, c1)
    long c0, c1;
    bool dt_word_ok;       // the previous step left the dt MIN in the slot's word
    TileLast tile_prev;    // lean_tile_last of the previous step
  };
  struct StepDone {
    unsigned nres;         // workgroups that wrote residual partials
    int nres_waves;        // ... and partials per workgroup
    bool exchanged;        // the new state's halo and the dt MIN are done (fused or overlapped)
  };
  StepPath step_path(const StepParams& P) const;   // (P completed: ny, sm)
  StepDone step_tile(StepCtx& c);
  StepDone step_lean_flat(const StepCtx& c);
  StepDone step_fused_euler(const StepCtx& c);
  StepDone step_lean_ns(const StepCtx& c);   // (with its entry step)
  StepDone lnm_step(const StepCtx& c);       // (likewise)
  StepDone step_split(const StepCtx& c, bool to_lns);
  void wall_heat(const StepCtx& c);          // wall heat transfer after the step (non-adiabatic walls)
  // mailbox transport, multi-workgroup kernels: a list's edge columns into the
  // neighbours' mailboxes, the publishing tail alone, mailbox -> ghost columns
  void p2p_push(const struct ColList& L, void* on_stream, int dt_slot, int fold_dt, int finish);
  void p2p_finish(int dt_slot);
  void p2p_unpack(const struct ColList& L, void* on_stream);
  // edge-first steps of the host transports: the comm stream and its events;
  // the edge part's halo (after ev_edge) on that stream, the dt MIN after it
  void overlap_streams();
  void overlap_exchange(int group, int slot_next);
  // fused lean N-S / mechanism steps: the HALO_LNS list of the post-step
  // buffers, and the previous step's list for the edge tiles' ghost prologue
  // (nullptr: p2p_complete unpacks it)
  void halo_fields_lns(std::vector<real*>& f, std::vector<unsigned char>& o, int sb, int pb, int cb, int ds) const;
  struct ColList lns_post_list(const char* what) const;
  const struct ColList* claim_ghost_prologue();
  bool lns_step_ok(const StepParams& P) const;
  bool lns_entry(const StepParams& P0) const;
  bool lnm_step_ok(const StepParams& P) const;
  void lnm_launch(const StepParams& P, const LnmArrays& a, const LeanTile& T, bool want_res, int slot, int slot_next,
                  int serial, unsigned ntile);
  // mechanism-mode kinetics of cells [k0, k1) (chem_fast / chem_mech / generic)
  void launch_chem(const StepParams& P, const SoA& mid, const SoA& out, long k0, long k1, unsigned nb, int slot);
};

std::unique_ptr<SolverBase> make_gpu_solver(Case& cs, int device);
std::unique_ptr<SolverBase> make_gpu_strip_solver(Case& cs, int device, int gi0, int gi1, Comm& boot,
                                                  const std::string& transport, std::string& used);

}  // namespace hf2d
