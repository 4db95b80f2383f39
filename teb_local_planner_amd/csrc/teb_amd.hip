// teb_amd.hip — libteb_amd.so: host side of the C-ABI declared in include/teb_amd.h (+ teb_amd_debug.h).
// Plain HIP runtime; no torch, no oracle, no CPU fallback: every entry point fails loudly without a gfx950 GPU.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <unistd.h>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <limits>
#include <string>
#include <random>
#include <vector>

#include "../../include/teb_amd.h"
#include "../../include/teb_amd_debug.h"
#define TEB_AMD_MAIN_TU   // (non-template kernels of the shared headers are defined here only)
#include "teb_kernel.hpp"
#include "teb_opt_launch.hpp"
#include "teb_fleet.hpp"
#include "teb_strip.hpp"
#include "teb_hsig.hpp"
#include "teb_graph.hpp"
#include "teb_comm.hpp"
#include "teb_rtc.hpp"
#include "teb_feasibility.hpp"
#include "teb_costmap_obstacles.hpp"
#include "teb_costmap_polygons.hpp"
#include "teb_plan_window.hpp"
#include "teb_scene_store.hpp"
#include "teb_band_store.hpp"
#include "teb_hcp_host.hpp"
#include "teb_costmap_host.hpp"
#include "teb_launch_host.hpp"
#include "teb_fleet_host.hpp"

using namespace tebamd;

// the two primitives of DevBuf (teb_scene_store.hpp)
tebamd::DevError tebamd::device_allocate(void** p, size_t bytes) { return hipMalloc(p, bytes); }
void tebamd::device_free(void* p) { (void)hipFree(p); }

// teb_launch_host.hpp names the layouts, the scene kinds and the limits of its rules itself: they are the kernel's
static_assert(LAYOUT_BAND == SOLVER_BAND && LAYOUT_BLOCKS == SOLVER_CR && LAYOUT_BAND_HBM == SOLVER_BANDG, "teb_launch_host.hpp numbers the layouts");
static_assert(KIND_POINTS == SCENE_POINTS && KIND_GENERIC == SCENE_GENERIC && KIND_POINTS_SMALL == SCENE_POINTS_SMALL && KIND_GENERIC_SMALL == SCENE_GENERIC_SMALL &&
              KIND_POINTS_DEFAULTS == SCENE_POINTS_DEFAULTS && KIND_POINTS_SMALL_DEFAULTS == SCENE_POINTS_SMALL_DEFAULTS && KIND_GENERIC_DEFAULTS == SCENE_GENERIC_DEFAULTS &&
              KIND_GENERIC_SMALL_DEFAULTS == SCENE_GENERIC_SMALL_DEFAULTS && KIND_POINTS_WIDE == SCENE_POINTS_WIDE && KIND_POINTS_SMALL_WIDE == SCENE_POINTS_SMALL_WIDE &&
              KIND_POINTS_LIGHT == SCENE_POINTS_LIGHT && KIND_POINTS_SMALL_LIGHT == SCENE_POINTS_SMALL_LIGHT && KIND_POINTS_CUSTOM == SCENE_POINTS_CUSTOM &&
              KIND_POINTS_SMALL_CUSTOM == SCENE_POINTS_SMALL_CUSTOM && KIND_GENERIC_CUSTOM == SCENE_GENERIC_CUSTOM && KIND_GENERIC_SMALL_CUSTOM == SCENE_GENERIC_SMALL_CUSTOM,
              "teb_launch_host.hpp numbers the scene kinds");
static_assert(kMaxSolverHelpers == kMcuMaxSpec, "teb_launch_host.hpp: one solver helper per speculative trial of teb_multicu.hpp");

// the instantiations of teb_optimize_kernel live in translation units of their own (teb_opt_launch.hpp)
TEB_OPT_FOR_ALL(TEB_OPT_DECLARE)
#ifdef TEB_AMD_SINGLE_TU
TEB_OPT_FOR_ALL(TEB_OPT_DEFINE)
#endif
// the fleet units (teb_fleet.hpp) are part of the product library only (build.py passes -DTEB_AMD_HAS_FLEET_UNITS with them)
#ifdef TEB_AMD_HAS_FLEET_UNITS
TEB_FLEET_FOR_ALL(TEB_FLEET_DECLARE)
#endif

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define HIPCHK(expr)                                                                                   \
  do {                                                                                                 \
    hipError_t _e = (expr);                                                                            \
    if (_e != hipSuccess)                                                                              \
      return fail(TEB_AMD_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(_e));               \
  } while (0)
// a kernel launch (the arguments of hipLaunchKernelGGL) and its launch error
#define LAUNCH(...) do { hipLaunchKernelGGL(__VA_ARGS__); HIPCHK(hipGetLastError()); } while (0)

// K9: selectBestTeb on the resident cost array (src/homotopy_class_planner.cpp:564-667)
__global__ void select_best_kernel(const double* cost, int count, int last_best, int initial_plan, double hyst,
                                   double prefer, double* out_cost, int* out_idx) {
  __shared__ double sv[kThreads];
  __shared__ int si[kThreads];
  double best = 1.7976931348623157e308;   // min_cost starts at numeric_limits<double>::max(), strict '<'
  int bi = -1;
  for (int i = threadIdx.x; i < count; i += kThreads) {
    double cst = cost[i];
    if (i == last_best) cst = cst * hyst;
    else if (i == initial_plan) cst = cst * prefer;
    if (cst < best) { best = cst; bi = i; }
  }
  sv[threadIdx.x] = best; si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) {
      double ov = sv[threadIdx.x + s]; int oi = si[threadIdx.x + s];
      double mv = sv[threadIdx.x]; int mi = si[threadIdx.x];
      bool take = (oi >= 0) && (mi < 0 || ov < mv || (ov == mv && oi < mi));
      if (take) { sv[threadIdx.x] = ov; si[threadIdx.x] = oi; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out_cost[0] = sv[0]; out_cost[1] = (double)si[0]; *out_idx = si[0]; }   // (cost, index) also as one 16-byte record
}

// debug: known-byte-count stream with the kernel's own global access pattern (8 B per lane, coalesced) used to
// calibrate rocprofv3's FETCH_SIZE / WRITE_SIZE on gfx950 (MI355X_MICROARCH.md, HBM section)
__global__ void stream_kernel(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i] + 1.0;
}

// debug: footprint_distance for a list of queries
__global__ void distance_kernel(const teb_amd_config_t c, const SceneDev sc, int nq, const int* oi, const double* x,
                                const double* y, const double* th, const int* st, const double* t, double* dist,
                                double* grad) {
  int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  double g[3];
  dist[q] = footprint_distance(c, sc, oi[q], x[q], y[q], cos(th[q]), sin(th[q]), st[q] != 0, t[q], g);
  grad[3 * q] = g[0]; grad[3 * q + 1] = g[1]; grad[3 * q + 2] = g[2];
}

}  // namespace

// The distance path and the layout chosen for the tables of a scene store (choose_scene_layout).
struct SceneLayout {
  int solver = 0;        // SOLVER_*
  int fast_points = 0;   // SCENE_POINTS: every table and the footprint point-like and the cache of the largest table fits the LDS
  int max_cache = 0;     // most rows of a table: what the obstacle cache of the LDS plan is made for
  LdsPlan plan;
  int cache_entries() const { return fast_points ? max_cache : 0; }   // 0: generic distance path
};

// What a handle owns beside device memory. Each frees what it holds, if anything; none is copied.
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() = default;
  OwnedStream(const OwnedStream&) = delete;
  ~OwnedStream() { if (s) (void)hipStreamDestroy(s); }
};
struct OwnedEvent {
  hipEvent_t e = nullptr;
  OwnedEvent() = default;
  OwnedEvent(const OwnedEvent&) = delete;
  ~OwnedEvent() { if (e) (void)hipEventDestroy(e); }
};
template <typename T>
struct PinnedBlock {   // hipHostMalloc
  T* p = nullptr;
  PinnedBlock() = default;
  PinnedBlock(const PinnedBlock&) = delete;
  ~PinnedBlock() { if (p) (void)hipHostFree(p); }
};

// TEARDOWN ORDER ("Who owns device memory"): the destructor body selects the device and waits for the stream; then the
// members go in reverse order of declaration - every DevBuf first, then the pinned blocks, the events and an owned stream, which
// therefore stand BEFORE every buffer below. teb_amd_destroy is `delete`.
struct teb_amd_handle {
  ~teb_amd_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
  }
  int device = 0;
  OwnedStream own_stream;         // the stream the handle made itself, if the caller passed none
  hipStream_t stream = nullptr;   // the stream everything runs on: the caller's, or own_stream.s
  OwnedEvent ev1, ev0;
  PinnedBlock<double> pack_host;   // the pinned host side of pack_dev
  PinnedBlock<unsigned> mcu_trace; // teb_amd_debug_mcu_watchdog: host-pinned breadcrumbs of the multi-CU launch, one word per workgroup
  teb_amd_config_t cfg;
  int max_tebs = 0, stride = 0, max_obst = 0, max_verts = 0, max_via = 0;
  int B = 0, M = 0, nvia = 0, n_static = 0, n_dyn = 0;
  int solver_created = 0;   // the layout chosen by teb_amd_create; teb_amd_set_obstacles may move a band to HBM (layout.solver)
  size_t hmat_stride = 0;
  int band_ldlt = 0;   // SOLVER_BAND: 1 = sequential banded LDL^T (teb_amd_options_t::band_ldlt), 0 = hybrid cyclic reduction
  size_t lds_limit = 0;
  int num_cus = 0;
  SceneLayout layout;   // of the single scene
  int static_radius_zero = 0;   // every obstacle of the static list enters the LDS cache with radius 0 (no circular obstacle among them)
  int last_defaults_profile = 0;   // the last optimise launch ran a *_DEFAULTS instantiation (teb_amd_debug_last_config_profile)
  int last_inst[3] = {-1, -1, -1}; // (layout, Jacobian mode, scene kind) of the instantiation the last optimise launch ran (teb_amd_debug_last_instantiation)
  teb_amd_options_t opt;   // behaviour switches fixed at create (ABI 2; never the process environment)
  int last_inner = 0;      // iterations_innerloop of the last teb_amd_optimize_batch (hasDiverged: size of g2o's batch statistics)
  int snap_nmax = -1;      // nmax_known at the time of teb_amd_snapshot_state
  int snap_B = -1;         // B at that time (the bound covers those bands only)
  int nmax_known = -1;     // upper bound of the resident pose counts as far as the host knows it, -1 = unknown (device-side producers ran)
  // the single scene (teb_scene_store.hpp): host copy of the last obstacle table - teb_amd_set_config re-derives the static / dynamic
  // lists from it, candidate generation reads its centroids -, the static list derived from it, and its device store
  HostObst hob;
  std::vector<int> host_static;
  DevSceneStore scene;
  // the batch (teb_band_store.hpp): the bands the kernels work on, the scratch compact_by_map gathers them through (allocated at the
  // first compaction), their strips from before a checked launch (allocated at the first one) and at the last snapshot
  DevBandStore bands, tmp;
  BandStrips ob, snap;
  Strips live() const { return bands.strips.view(); }
  Strips saved() const { return ob.view(); }
  Strips snapshot() const { return snap.view(); }
  // the scratch of an optimise launch, BatchDev's beyond the bands
  DevBuf<int> assoc_cnt, assoc, assoc_ovf, via_pose, legacy_idx;
  DevBuf<double> Hbackup, Hband;
  DevBuf<long long> clk;   // BatchDev::clk
  // multi-CU mode (teb_multicu.hpp): control words, published poses, distance records; sized on first use
  DevBuf<unsigned> mcu_ctl;
  DevBuf<double> pack_dev;          // packed messages of small batches (kPackMaxDoubles)
  DevBuf<double> mcu_pub, mcu_items, mcu_spec;
  size_t mcu_items_have = 0;
  int mcu_last_helpers = 0;   // distance helpers per band of the last launch (0: none), teb_amd_last_launch_info
  int mcu_last_solvers = 0;   // solver helpers per band of the last launch
  int mcu_last_repeated = 0;  // that launch timed out waiting for its helpers and was repeated on one CU per band
  HelperBackoff mcu_backoff;  // the pause of the distance helpers after a launch they came late to (teb_launch_host.hpp)
  int mcu_watchdog_ms = 0;
  int mcu_debug_flags = 0;
  DevBuf<double> iter_log;   // teb_amd_set_iteration_log: [max_tebs][TEB_AMD_ITERATION_LOG_ROWS][4]
  bool iter_log_on = false;
  DevBuf<double> phase_log;  // teb_amd_set_phase_log: [max_tebs][kPhaseLogSlots]
  bool phase_log_on = false;
  size_t hband_stride = 0;
  // debug / select
  DevBuf<double> dbg_H, dbg_b, dbg_chi2, sel_cost;
  DevBuf<int> sel_idx, err_flag;
  // strip producers / consumers (f1, f2)
  DevBuf<double> stage_x, stage_y, stage_yaw, out_cmd, out_prof, out_traj;
  bool consumers_valid = false;
  // equivalence classes (f3)
  DevBuf<double> hsig, hs_pre, hs_pim;
  DevBuf<int> hs_pex;
  SignatureSet sigs;            // of the single scene's bands (teb_hcp_host.hpp); hsig is the scratch of every signature launch
  bool hs_prod_valid = false;   // hs_pre / hs_pim / hs_pex hold the products of the current obstacle table
  int consumers_la = 0, consumers_prevent = 0;
  bool timed = false;
  // candidate generation (f3): graph + candidate scratch strips, boost-compatible generator
  BandStrips cand;   // kCandChunk candidate bands; allocated with the scratch below (ensure_candidate_buffers)
  DevBuf<double> g_vx, g_vy, cand_sig, cand_px, cand_py;
  DevBuf<int> cand_off, cand_map;
  DevBuf<unsigned char> g_adj;
  PlannerMemory memory;   // what the single scene's planner remembers between ticks (teb_hcp_host.hpp); g_vx .. g_adj above are launch scratch
  // costmap (f4)
  DevBuf<unsigned char> cm_cells;
  DevBuf<double> cm_fp;
  DevBuf<int> cm_out;
  GridDev cm{};   // the single costmap (teb_amd_set_costmap) over cm_cells; sx = 0: none
  // the costmap set (teb_amd_set_costmaps): one grid per scene of a fleet, beside the single costmap above, which it never touches. The
  // grids lie one after the other in ONE buffer; grids_host holds the GridDev records of the device array (device pointers).
  struct CostmapSet {
    int n = 0;   // 0 = none
    DevBuf<unsigned char> cells;
    DevBuf<GridDev> grids;
    std::vector<GridDev> grids_host;
  } cms;
  // scratch of the costmap conversion (convert_costmaps), shared by its two row kinds and two routes
  struct CostmapScratch {
    // point route: kept cells per lane, then their offsets + a total per scene; of a set also the records and totals of the scenes
    // (max_tebs each, allocated once) and the points of the write pass (max_obstacles, allocated once)
    DevBuf<int> cnt, tot;
    DevBuf<CmoSceneRec> rec;
    DevBuf<double> px, py;
    // polygon route: rows / vertices / polygon vertices per block (then their offsets + totals) and the converted rows (first-vertex
    // offsets, vertex coordinates) before the host builds the tables from them; of a set also the records of the scenes, the prefix
    // array of their block counts and the 3 x n_scenes totals (by max_tebs, allocated once)
    DevBuf<int> pcnt, poff, blk, ptot;
    DevBuf<CmpSceneRec> prec;
    DevBuf<double> pvx, pvy;
  } cmx;
  // scratch of the per-scene calls at the far end of a fleet tick: the bands of teb_amd_is_trajectory_feasible_per_scene, the message
  // of teb_amd_update_and_prune_per_scene
  DevBuf<int> cms_bands;
  DevBuf<double> prune_msg;
  DevBuf<FeasSpecDev> cms_specs;   // the record of every scene of teb_amd_is_trajectory_feasible_per_class
  // the global plans (teb_amd_set_global_plans): the plans of every robot one after the other in ONE buffer (x | y | yaw planes of
  // `total` poses), their first poses, counts and pruning cursors, and the scratch of teb_amd_plan_windows: the poses / transforms /
  // thresholds of a call, the per-robot records, the pack buffer of the windows and via-points and its ticket. Beside the costmap set
  // and the scene set; touches neither.
  struct PlanSet {
    int n = 0;   // 0 = none
    size_t total = 0;
    DevBuf<double> poses, in, pack;
    DevBuf<long long> first;
    DevBuf<int> count, cursor;
    DevBuf<PlanWinOut> rec;
    DevBuf<unsigned long long> ticket;
    std::vector<int> count_host;
  } plans;
  // fleet batches (teb_fleet.hpp, teb_amd_set_scenes): the scene set - a second DevSceneStore, allocated at the first
  // teb_amd_set_scenes and sized by the capacities of the handle, with the rows, vertices and via-points of the scenes one after the
  // other (scene_segments) - and what a fleet launch needs beside it
  struct FleetStorage {   // the device side of the scene set
    DevSceneStore store;
    DevBuf<int> scene_of, sel_last, sel_init, sel_idx;
    DevBuf<double> sel_cost;
    DevBuf<SceneDev> scenes;
    // the table of robot classes a fleet launch reads (upload_class_table, the install, and nothing else writes them): the classes of
    // the map and the class of every scene, or ONE class - the handle's configuration - and zeros [max_tebs]
    DevBuf<teb_amd_config_t> cfgs;
    DevBuf<int> class_of_scene;
    // equivalence classes per scene (teb_amd_compute_h_signatures_per_scene): state of the scene set, beside the single scene's
    // (sigs, hs_pre .. above), which the per-scene calls never touch
    DevBuf<double> hs_pre, hs_pim;   // 2-D: prod_l of every row of the set's store, each over the rows of its own scene
    DevBuf<int> hs_pex, hs_off;      // hs_off [max_tebs + 1]: first value of every band in the signature buffer
    // scratch of the candidate exploration per scene, separate from the single scene's and allocated at the first call: candidate
    // strips, path points, offsets, candidate -> scene map, signatures; the graphs of a call (vertices, adjacency, records)
    BandStrips ex;
    DevBuf<double> ex_px, ex_py, ex_pyaw, ex_sig, ex_orient, ex_line, ex_gvx, ex_gvy;
    DevBuf<int> ex_off, ex_scene, ex_soff, ex_map;
    DevBuf<unsigned char> ex_gadj;
    DevBuf<GraphFleetRec> ex_rec;
  };
  struct Fleet : FleetStorage {
    int n_scenes = 0;               // 0 = single-scene mode
    bool allocated = false;
    std::vector<HostObst> tabs;     // host copy of every scene's table: teb_amd_set_config re-derives the lists from them
    std::vector<int> via_count;
    // the class map (teb_amd_set_scene_configs): a configuration per robot class and the class of every scene; both empty = none, every
    // scene runs under h->cfg. It has the lifetime of the scene count (forget_classes where new_planners forgets).
    std::vector<teb_amd_config_t> classes;
    std::vector<int> class_of;
    std::vector<int> band_scene;   // [max_tebs] scene of every band (teb_amd_set_band_scenes); survives set / clear
    SceneLayout layout;             // of a fleet launch (the single-scene choice h->layout is not touched)
    bool hs_prod_valid = false;
    SignatureSet sigs;               // of the bands of the set, each as wide as its scene's table
    std::vector<PlannerMemory> memory;   // [n_scenes] what the planner of every scene - a robot - remembers; none of it is the single scene's
    void new_planners(size_t ns) { memory.assign(ns, PlannerMemory()); }   // ns planners that remember nothing
    void release() { static_cast<FleetStorage&>(*this) = FleetStorage(); allocated = false; }   // the device side
  } fleet;
  int explore_quota = 0;   // teb_amd_debug_set_explore_quota: paths per scene and round of the per-scene exploration, 0 = kExploreQuota
  // the bands, the obstacles or the configuration change: the signatures of an earlier compute call are stale, the single scene's and
  // the scene set's alike
  void signatures_stale() { sigs.clear(); fleet.sigs.clear(); }
  // the bands changed on the device: the consumers' outputs are void, the host's bound on the pose counts is nmax (-1: unknown) and,
  // unless the caller moves the signatures with the bands, these are stale
  void bands_changed(int nmax = -1, bool signatures_too = true) { consumers_valid = false; nmax_known = nmax; if (signatures_too) signatures_stale(); }
};

namespace {

int check_handle(teb_amd_handle* h) {
  if (!h) return fail(TEB_AMD_ERR_INVALID_ARG, "null handle");
  if (hipSetDevice(h->device) != hipSuccess) return fail(TEB_AMD_ERR_HIP, "hipSetDevice failed");
  return TEB_AMD_OK;
}

int synced(teb_amd_handle* h) {
  HIPCHK(hipStreamSynchronize(h->stream));
  return TEB_AMD_OK;
}

SceneDev scene_of(teb_amd_handle* h) {
  return h->scene.view(SceneSegment{}, h->M, h->nvia, h->n_static, h->n_dyn, h->static_radius_zero, h->layout.fast_points);
}

BatchDev batch_of(teb_amd_handle* h) {
  BatchDev b;
  b.B = h->B; b.stride = h->stride;
  h->bands.view(b);
  b.assoc_cnt = h->assoc_cnt.p; b.assoc = h->assoc.p; b.assoc_cap = h->max_obst > 0 ? h->max_obst : 1;
  b.assoc_overflow = h->assoc_ovf.p; b.legacy_idx = h->legacy_idx.p;
  b.via_pose = h->via_pose.p; b.via_cap = h->max_via > 0 ? h->max_via : 1;
  b.Hbackup = h->Hbackup.p; b.hmat_stride = h->hmat_stride;
  b.clk = h->clk.p;
  return b;
}

// The class list something runs under (teb_fleet_host.hpp states the rules over it): the map of teb_amd_set_scene_configs with the class
// of every scene, or ONE class - the handle's configuration - for every scene (class_of null). The single scene of the handle always
// runs under own_class.
struct ClassList {
  const teb_amd_config_t* cfgs;
  int n;
  const int* class_of;   // [n_scenes], null: class 0
  const teb_amd_config_t& of_scene(size_t s) const { return cfgs[class_of ? class_of[s] : 0]; }
};
ClassList own_class(const teb_amd_handle* h) { return ClassList{&h->cfg, 1, nullptr}; }
ClassList fleet_classes(const teb_amd_handle* h) {
  const auto& F = h->fleet;
  return F.classes.empty() ? own_class(h) : ClassList{F.classes.data(), (int)F.classes.size(), F.class_of.data()};
}
// what the current mode runs under: the scene set's list in fleet mode, the handle's configuration else
ClassList live_classes(const teb_amd_handle* h) { return h->fleet.n_scenes > 0 ? fleet_classes(h) : own_class(h); }
// the configuration band b runs under: that of its scene's class in fleet mode (a band whose scene is not in the set: the handle's)
const teb_amd_config_t& band_cfg(const teb_amd_handle* h, int b) {
  const auto& F = h->fleet;
  if (F.n_scenes <= 0 || (size_t)b >= F.band_scene.size() || F.band_scene[b] >= F.n_scenes) return h->cfg;
  return fleet_classes(h).of_scene((size_t)F.band_scene[b]);
}
// a field the classes of one list agree on (fleet_classes_agree), for the scene set (by_scene) or the single scene
const teb_amd_config_t& agreed_cfg(const teb_amd_handle* h, bool by_scene) { return by_scene ? fleet_classes(h).cfgs[0] : h->cfg; }

int validate_config(const teb_amd_config_t* c) {
  if (c->footprint_type < TEB_AMD_FOOTPRINT_POINT || c->footprint_type > TEB_AMD_FOOTPRINT_POLYGON)
    return fail(TEB_AMD_ERR_INVALID_ARG, "unknown footprint_type");
  if (c->footprint_type == TEB_AMD_FOOTPRINT_LINE && c->footprint_n_vertices != 2)
    return fail(TEB_AMD_ERR_INVALID_ARG, "line footprint needs exactly 2 vertices");
  if (c->footprint_type == TEB_AMD_FOOTPRINT_POLYGON &&
      (c->footprint_n_vertices < 1 || c->footprint_n_vertices > TEB_AMD_MAX_FOOTPRINT_VERTICES))
    return fail(TEB_AMD_ERR_INVALID_ARG, "polygon footprint needs 1..64 vertices");
  if (c->jacobian_mode != TEB_AMD_JACOBIAN_ANALYTIC && c->jacobian_mode != TEB_AMD_JACOBIAN_G2O_NUMERIC)
    return fail(TEB_AMD_ERR_INVALID_ARG, "jacobian_mode must be TEB_AMD_JACOBIAN_ANALYTIC or TEB_AMD_JACOBIAN_G2O_NUMERIC");
  return TEB_AMD_OK;
}

const void* opt_kernel(int solver, int jmode, int scene) {
#define TEB_OPT_PICK(S, J, P) if (solver == S && jmode == J && scene == P) return TEB_OPT_KERNEL_FN(S, J, P)();
  TEB_OPT_FOR_ALL(TEB_OPT_PICK)
#undef TEB_OPT_PICK
  return nullptr;   // (a -DTEB_AMD_ANALYTIC_ONLY build asked for the numeric mode)
}
// Which specialised instantiation may run this launch: 1 = the *_DEFAULTS kinds (every flag of the profile table folded), 2 = the *_WIDE
// kinds (point-like scenes: every fold but the via-points and the holonomic choice), 3 = the *_LIGHT kinds (point-like scenes: every
// cost-term flag at run time, only the never-reached bulk folded), 0 = none (generic instantiation). GENERATED from the
// table of teb_device.hpp (TEB_PF_ALL): a flag is folded in the kernel exactly when its TEB_PF_HOST_<ID> condition is required here, so a
// fold cannot exist without its host-side check (tests/test_config_profile_sites.py). `c`, `args`, `sc` are the names the table's
// expressions use - the very objects the kernel is launched with.
int profile_matches(const teb_amd_handle* h, const OptArgs& args, const SceneDev& sc) {
  if (h->opt.generic_config_path) return 0;
  const teb_amd_config_t& c = h->cfg;
  const bool points = sc.fast_points != 0;   // (generic-shape kinds keep the TEB_PF_KIN_* flags at run time)
  bool narrow = true, wide = true, light = true;
#define TEB_PF_CHECK(ID)                                                        \
  if ((points || !TEB_PF_KIN_##ID) && !(TEB_PF_HOST_##ID)) {                    \
    narrow = false;                                                             \
    if (!TEB_PF_WIDE_##ID) wide = false;                                        \
    if (!TEB_PF_LIGHT_##ID) light = false;                                      \
  }
  TEB_PF_ALL(TEB_PF_CHECK)
#undef TEB_PF_CHECK
  return narrow ? 1 : (wide && points ? 2 : (light && points ? 3 : 0));
}
// The instantiation compiled at run time for this launch (teb_amd_options_t::compile_for_config), READY, or null: not asked for, a default
// configuration (pf == 1: its pre-built kernel IS the fully folded one), not ready yet, or failed. wait: block until the compiler is done.
std::shared_ptr<RtcKernel> rtc_lookup(const teb_amd_handle* h, const OptArgs& args, const SceneDev& sc, int solver, bool small, int pf, bool wait) {
  if (!((pf != 1 || h->opt.compile_for_config >= 3) && h->opt.compile_for_config > 0 && !h->opt.generic_config_path && !args.debug_linearize)) return nullptr;   // (3: even for a default configuration - measurement only)
  const teb_amd_config_t& c = h->cfg;
#ifdef TEB_AMD_ANALYTIC_ONLY
  if (c.jacobian_mode != TEB_AMD_JACOBIAN_ANALYTIC) return nullptr;   // this variant has no numeric mode: the run-time compiler must not add one
#endif
  RtcKey key;
  key.flags = 0;
  int bit = 0;
#define TEB_PF_BIT(ID) key.flags |= (unsigned long long)((TEB_PF_EXPR_##ID) ? 1 : 0) << bit; ++bit;
  TEB_PF_ALL(TEB_PF_BIT)
#undef TEB_PF_BIT
  key.solver = solver; key.jmode = c.jacobian_mode;
  key.scene = scene_kinds(pf, sc.fast_points != 0, small, c.jacobian_mode).custom;
  if (key.scene == KIND_NONE) return nullptr;   // (helper workgroups exist in the small-batch kinds only, which exist for closed-form Jacobians)
  std::string why;
  std::shared_ptr<RtcKernel> rk = rtc_request(key, wait, &why);
  return (rk && rk->state.load() == RtcKernel::READY) ? rk : nullptr;
}
// The fleet units (teb_fleet.hpp): closed-form Jacobians, SCENE_POINTS / SCENE_GENERIC. Null in the variants built without them.
const void* fleet_kernel(int solver, int scene) {
#ifdef TEB_AMD_HAS_FLEET_UNITS
#define TEB_FLEET_PICK(S, P) if (solver == S && scene == P) return TEB_FLEET_KERNEL_FN(S, P)();
  TEB_FLEET_FOR_ALL(TEB_FLEET_PICK)
#undef TEB_FLEET_PICK
#endif
  (void)solver; (void)scene;
  return nullptr;
}
// one workgroup per band, every band against fleet.scenes[fleet.scene_of[b]] under the configuration of that scene's class: no helper
// workgroups, no run-time compilation
hipError_t launch_fleet(teb_amd_handle* h, int grid, const BatchDev& bt, const OptArgs& a, int solver, const LdsPlan& plan) {
  const int scene_kind = h->fleet.layout.fast_points ? SCENE_POINTS : SCENE_GENERIC;
  const void* k = fleet_kernel(solver, scene_kind);
  h->last_defaults_profile = 0;
  h->last_inst[0] = solver; h->last_inst[1] = TEB_AMD_JACOBIAN_ANALYTIC; h->last_inst[2] = -1;
  if (!k) return hipErrorInvalidDeviceFunction;
  h->last_inst[2] = scene_kind;
  FleetDev fl;
  fl.scenes = h->fleet.scenes.p; fl.scene_of = h->fleet.scene_of.p;
  McuDev none;
  std::memset(&none, 0, sizeof none);
  const teb_amd_config_t* cfgs = h->fleet.cfgs.p;   // the class table (upload_class_table): the map's, or the handle's configuration alone
  const int* class_of_scene = h->fleet.class_of_scene.p;
  void* params[] = {&fl, const_cast<BatchDev*>(&bt), const_cast<OptArgs*>(&a), const_cast<LdsPlan*>(&plan), &none, &cfgs, &class_of_scene};
  return hipLaunchKernel(k, dim3(grid), dim3(kThreads), params, plan.total_bytes, h->stream);
}
// one workgroup per band (and its helper workgroups, mcu) against the scene sc, in the layout `solver` with its LDS plan
hipError_t launch_opt(teb_amd_handle* h, int grid, const SceneDev& sc, const BatchDev& bt, const OptArgs& a, int solver, const LdsPlan& plan,
                      const McuDev* mcu = nullptr) {
  McuDev none;
  std::memset(&none, 0, sizeof none);
  const McuDev* mc = mcu ? mcu : &none;
  const bool small = mc->K + mc->D > 0;   // helper workgroups: the small-batch instantiation of the scene kind
  const int pf = profile_matches(h, a, sc);
  const SceneKinds kinds = scene_kinds(pf, sc.fast_points != 0, small, h->cfg.jacobian_mode);
  h->last_defaults_profile = 0;
  h->last_inst[0] = solver; h->last_inst[1] = h->cfg.jacobian_mode; h->last_inst[2] = -1;   // which instantiation runs (teb_amd_debug_last_instantiation)
  void* params[] = {const_cast<teb_amd_config_t*>(&h->cfg), const_cast<SceneDev*>(&sc), const_cast<BatchDev*>(&bt), const_cast<OptArgs*>(&a),
                    const_cast<LdsPlan*>(&plan), const_cast<McuDev*>(mc)};
  // a configuration off the defaults: the instantiation compiled for IT at run time, once it is ready (teb_rtc.hpp)
  if (std::shared_ptr<RtcKernel> rk = rtc_lookup(h, a, sc, solver, small, pf, false)) {
    std::string why;
    hipFunction_t f = rtc_function(*rk, h->device, h->lds_limit, &why);
    if (f) {
      h->last_defaults_profile = 4;
      h->last_inst[2] = kinds.custom;
      return hipModuleLaunchKernel(f, grid * (1 + mc->K + mc->D), 1, 1, kThreads, 1, 1, plan.total_bytes, h->stream, params, nullptr);
    }
  }
  const Prebuilt pre = pick_prebuilt(kinds, pf, [&](int kind) { return opt_kernel(solver, h->cfg.jacobian_mode, kind); });
  if (!pre.fn) return hipErrorInvalidDeviceFunction;
  h->last_defaults_profile = pre.profile;
  h->last_inst[2] = pre.kind;
  return hipLaunchKernel(pre.fn, dim3(grid * (1 + mc->K + mc->D)), dim3(kThreads), params, plan.total_bytes, h->stream);
}

// bytes(S, layout, cache entries) of the LDS plan on a device whose workgroups may use lds_limit bytes: what the rules of teb_launch_host.hpp ask
auto plan_bytes_of(size_t lds_limit) {
  return [lds_limit](int S, int solver, int ob) { return (size_t)make_lds_plan(S, solver, ob, lds_limit).total_bytes; };
}
// what helpers_wanted reads of the handle and the call (h->layout, h->M: helpers exist against the single scene only)
HelperInputs helper_inputs(const teb_amd_handle* h, const OptArgs& args, bool fleet, int layout) {
  HelperInputs in;
  in.fleet = fleet; in.debug_linearize = args.debug_linearize != 0; in.jacobian_mode = h->cfg.jacobian_mode;
  in.B = h->B; in.M = h->M; in.stride = h->stride; in.nmax_known = h->nmax_known; in.num_cus = h->num_cus;
  in.speculative_trials = h->opt.speculative_trials; in.multi_cu = h->opt.multi_cu;
  in.layout = layout; in.band_ldlt = h->band_ldlt != 0; in.inner = args.inner;
  in.fast_points = h->layout.fast_points != 0; in.legacy_association = h->cfg.legacy_obstacle_association != 0;
  return in;
}

// the four strips and the pose counts in ONE launch (five copy commands cost more in launch gaps than in bytes: 2.4 MB at the headline)
__global__ void __launch_bounds__(256) copy_state_kernel(double* __restrict__ x, double* __restrict__ y, double* __restrict__ th,
                                                         double* __restrict__ dt, int* __restrict__ n, const double* __restrict__ sx,
                                                         const double* __restrict__ sy, const double* __restrict__ sth,
                                                         const double* __restrict__ sdt, const int* __restrict__ sn, size_t count, int B) {
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step) {
    x[i] = sx[i]; y[i] = sy[i]; th[i] = sth[i]; dt[i] = sdt[i];
    if (i < (size_t)B) n[i] = sn[i];
  }
}
// Small batches (a planner tick, one TebOptimalPlanner): a dozen tiny copies cost more in host calls than in bytes. The bands and their
// attributes travel as ONE packed message through a pinned host buffer and ONE copy; these kernels scatter / gather it on the device.
// Message (doubles; the integer attributes are exact as doubles): [n | has_vs | has_vg | rotdir | via_en] B each, [vs | vg] 3 B each,
// then x | y | theta | dt, B rows of w columns each.
constexpr size_t kPackMaxDoubles = 65536;   // 512 KB: beyond that the strided copies win
__global__ void __launch_bounds__(256) unpack_bands_kernel(const double* __restrict__ msg, int B, int w, int S, int* n, int* hvs, int* hvg, int* rd, int* ve,
                                                           double* vs, double* vg, double* x, double* y, double* th, double* dt, int* optimized) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < B) { n[t] = (int)msg[t]; hvs[t] = (int)msg[B + t]; hvg[t] = (int)msg[2 * B + t]; rd[t] = (int)msg[3 * B + t]; ve[t] = (int)msg[4 * B + t]; optimized[t] = 0; }
  if (t < 3 * B) { vs[t] = msg[5 * B + t]; vg[t] = msg[8 * B + t]; }
  const double* body = msg + 11 * (size_t)B;
  const size_t plane = (size_t)B * w;
  for (size_t q = t; q < plane; q += (size_t)gridDim.x * blockDim.x) {
    const size_t b = q / w, i = q - b * w, o = b * S + i;
    x[o] = body[q]; y[o] = body[plane + q]; th[o] = body[2 * plane + q]; dt[o] = body[3 * plane + q];
  }
}
__global__ void __launch_bounds__(256) pack_bands_kernel(double* __restrict__ msg, int B, int w, int S, const int* n, const double* x, const double* y,
                                                         const double* th, const double* dt) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < B) msg[t] = (double)n[t];
  double* body = msg + B;
  const size_t plane = (size_t)B * w;
  for (size_t q = t; q < plane; q += (size_t)gridDim.x * blockDim.x) {
    const size_t b = q / w, i = q - b * w, o = b * S + i;
    body[q] = x[o]; body[plane + q] = y[o]; body[2 * plane + q] = th[o]; body[3 * plane + q] = dt[o];
  }
}
// [status | lm_iterations | lm_trials | chi2 | cost | lambda] B each
__global__ void __launch_bounds__(256) pack_results_kernel(double* __restrict__ msg, int B, const int* status, const int* iters, const int* trials, const double* chi2,
                                                           const double* cost, const double* lambda) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < B) { msg[t] = (double)status[t]; msg[B + t] = (double)iters[t]; msg[2 * B + t] = (double)trials[t]; msg[3 * B + t] = chi2[t]; msg[4 * B + t] = cost[t]; msg[5 * B + t] = lambda[t]; }
}

static int copy_strips(teb_amd_handle_t* h, const Strips& dst, const Strips& src, int bands) {
  const size_t count = (size_t)bands * h->stride;   // >= bands
  const int grid = (int)std::min<size_t>(2048, (count + 255) / 256);
  LAUNCH(copy_state_kernel, dim3(grid), dim3(256), 0, h->stream, dst.x, dst.y, dst.th, dst.dt, dst.n, src.x, src.y, src.th, src.dt, src.n, count, bands);
  return TEB_AMD_OK;
}

// The per-band flags of the launch that just ran - a band outgrew the layout (2), the helpers of the multi-CU mode came late (4) - and,
// if asked for, the longest band. Synchronous: the flags decide whether the launch has to be repeated (documented in teb_amd.h).
int read_flags(teb_amd_handle* h, bool* outgrown, bool* helpers_late, int* nmax) {
  std::vector<int> ovf(h->B), nn(nmax ? h->B : 0);
  HIPCHK(hipMemcpyAsync(ovf.data(), h->assoc_ovf.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (nmax) HIPCHK(hipMemcpyAsync(nn.data(), h->bands.strips.n.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int flags = 0;
  for (int v : ovf) flags |= v;
  *outgrown = (flags & 2) != 0;
  if (helpers_late) *helpers_late = (flags & 4) != 0;
  if (nmax) *nmax = nn.empty() ? 0 : std::max(0, *std::max_element(nn.begin(), nn.end()));
  return TEB_AMD_OK;
}
// diagnostic (teb_amd_debug_mcu_watchdog): a multi-CU launch that does not finish in time is reported with the breadcrumbs of its
// workgroups, and the process ends (a kernel cannot be cancelled; the bounded spins of the kernel make this unreachable unless the
// protocol itself is broken)
void mcu_watchdog(teb_amd_handle* h, int H) {
  const auto t0 = std::chrono::steady_clock::now();
  while (hipStreamQuery(h->stream) == hipErrorNotReady) {
    if (std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > h->mcu_watchdog_ms) {
      fprintf(stderr, "[teb_amd multi-CU watchdog] launch of %d bands x (1 + %d) workgroups still running after %d ms; breadcrumbs (epoch << 8 | code):\n", h->B, H, h->mcu_watchdog_ms);
      for (int w = 0; w < h->B * (1 + H) && w < 1024; ++w) fprintf(stderr, " wg%d:%x", w, h->mcu_trace.p[w]);
      fprintf(stderr, "\n");
      fflush(stderr);
      _exit(3);
    }
  }
}

// The buffers of the multi-CU mode for hp helpers per band, sized on first use, its control words zeroed on the stream before the
// launch, and what the kernel is told of them. A failed allocation of the distance records is no error: the launch then runs without
// distance helpers (hp.D = 0).
int prepare_helpers(teb_amd_handle* h, Helpers& hp, McuDev& mcu) {
  std::memset(&mcu, 0, sizeof mcu);
  const size_t need_items = hp.D > 0 ? distance_records(h->B, h->M, h->stride) : 0;
  if (h->mcu_items_have < need_items) {
    h->mcu_items.free(); h->mcu_items_have = 0;
    if (h->mcu_items.alloc(need_items) != hipSuccess) { (void)hipGetLastError(); hp.D = 0; }
    else h->mcu_items_have = need_items;
  }
  if (hp.K + hp.D == 0) return TEB_AMD_OK;
  if (!h->mcu_ctl.p) {
    HIPCHK(h->mcu_ctl.alloc((size_t)h->max_tebs * kMcuCtlWords)); HIPCHK(h->mcu_pub.alloc((size_t)h->max_tebs * kMcuPubArrays * h->stride));
    HIPCHK(h->mcu_spec.alloc((size_t)h->max_tebs * (kMcuMaxSpec + 1) * mcu_spec_slot(h->stride)));
  }
  HIPCHK(hipMemsetAsync(h->mcu_ctl.p, 0, (size_t)h->B * kMcuCtlWords * sizeof(unsigned), h->stream));
  mcu.K = hp.K; mcu.D = hp.D; mcu.ctl = h->mcu_ctl.p; mcu.pub = h->mcu_pub.p; mcu.items = hp.D > 0 ? h->mcu_items.p : nullptr; mcu.item_cap = h->M; mcu.spec = h->mcu_spec.p;
  mcu.timeout_ticks = helper_timeout_ticks(h->opt.multi_cu_timeout_us);
  if (hp.D > 0) mcu.timeout_ticks = h->mcu_backoff.probe_timeout(mcu.timeout_ticks);
  mcu.trace = h->mcu_trace.p;
  mcu.debug_flags = h->mcu_debug_flags;
  if (h->mcu_trace.p) std::memset(h->mcu_trace.p, 0, 1024 * sizeof(unsigned));
  return TEB_AMD_OK;
}
// the strips as they are now, for a repeat of the launch
int save_strips(teb_amd_handle* h) {
  if (!h->ob.bands()) HIPCHK(h->ob.alloc(h->max_tebs, h->stride));
  return copy_strips(h, h->saved(), h->live(), h->B);
}
// the longest resident band, read back from the device
int longest_band(teb_amd_handle* h, int* nmax) {
  std::vector<int> n(h->B);
  HIPCHK(hipMemcpyAsync(n.data(), h->bands.strips.n.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *nmax = 0;
  for (int v : n) *nmax = std::max(*nmax, v);
  return TEB_AMD_OK;
}

// One optimise launch: what it runs is decided by the rules of teb_launch_host.hpp; here are the buffers, the launches and the copies.
int launch(teb_amd_handle* h, const OptArgs& args) {
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs uploaded");
  // What the launch runs against, decided ONCE: the single scene of the handle, or the scene set (teb_amd_set_scenes) - then the layout,
  // the plan and the obstacle cache are those of the set (its largest scene).
  const bool fleet = h->fleet.n_scenes > 0;
  const SceneLayout& own = fleet ? h->fleet.layout : h->layout;
  SceneDev sc = scene_of(h);
  BatchDev bt = batch_of(h);
  // (a fleet launch has no helper workgroups: mcu is null then)
  auto run = [&](int solver, const LdsPlan& plan, const McuDev* mcu) {
    return fleet ? launch_fleet(h, h->B, bt, args, solver, plan) : launch_opt(h, h->B, sc, bt, args, solver, plan, mcu);
  };
  // 1. decide: the layout of this launch (layout_per_launch), its helper workgroups, whether its flags are looked at afterwards
  const LayoutSwitches sw{args.debug_linearize != 0, h->opt.fixed_layout != 0, h->opt.layout != TEB_AMD_LAYOUT_AUTO, h->band_ldlt != 0};
  int nmax = h->nmax_known;
  if (nmax < 0 && may_launch_optimistic(own.solver, sw))   // a device-side producer changed the bands since the host last saw their pose counts
    if (int rc = longest_band(h, &nmax)) return rc;
  const LaunchLayout lay = layout_per_launch(own.solver, sw, nmax, h->stride, own.cache_entries(), h->lds_limit, plan_bytes_of(h->lds_limit));
  const int eff_solver = lay.layout;
  const LdsPlan eff_plan = lay.optimistic ? make_lds_plan(lay.S, eff_solver, own.cache_entries(), h->lds_limit) : own.plan;
  Helpers hp = helpers_for_launch(helper_inputs(h, args, fleet, eff_solver), h->mcu_backoff);
  // 2. make sure the buffers exist (without distance records there are no distance helpers), 3. save the strips
  McuDev mcu;
  if (int rc = prepare_helpers(h, hp, mcu)) return rc;
  const int K = hp.K, D = hp.D, H = K + D;
  h->mcu_last_helpers = D; h->mcu_last_solvers = K; h->mcu_last_repeated = 0;
  const bool checked = launch_is_checked(lay.optimistic, D);
  if (checked)
    if (int rc = save_strips(h)) return rc;
  // 4. run
  if (h->opt.compile_for_config >= 2 && !fleet)   // synchronous mode: the wait for the compiler is not kernel time
    (void)rtc_lookup(h, args, sc, eff_solver, H > 0, profile_matches(h, args, sc), true);
  HIPCHK(hipEventRecord(h->ev0.e, h->stream));   // (the kernel clears its bands' overflow flags itself)
  HIPCHK(run(eff_solver, eff_plan, H > 0 ? &mcu : nullptr));
  if (H > 0 && h->mcu_trace.p && h->mcu_watchdog_ms > 0) mcu_watchdog(h, H);
  if (checked) {
    // 5. look at the flags, 6. ask the ladder, 7. run what it says - from the saved strips, without helpers; ev0 stays where it was: the
    // reported time includes the discarded launches
    HIPCHK(hipGetLastError());
    bool outgrown = false, helpers_late = false;
    if (int rc = read_flags(h, &outgrown, &helpers_late, &h->nmax_known)) return rc;
    if (D > 0) h->mcu_backoff.update(helpers_late);
    LadderStep step = after_first_look(lay.optimistic, outgrown, helpers_late);
    if (step.next == LadderStep::RETRY_OPTIMISTIC) {
      if (int crc = copy_strips(h, h->live(), h->saved(), h->B)) return crc;
      HIPCHK(run(eff_solver, eff_plan, nullptr));
      if (int rc = read_flags(h, &outgrown, nullptr, nullptr)) return rc;
      step = after_second_look(outgrown);
    }
    if (step.next == LadderStep::OWN_LAYOUT) {
      if (int crc = copy_strips(h, h->live(), h->saved(), h->B)) return crc;
      HIPCHK(run(own.solver, own.plan, nullptr));
    }
    h->mcu_last_repeated = step.repeated;
    if (step.nmax_stale) h->nmax_known = -1;
  } else if (fleet_any_autosize(live_classes(h).cfgs, live_classes(h).n) && !args.debug_linearize) {
    h->nmax_known = -1;   // asynchronous launch: autoResize may change the pose counts
  }
  h->consumers_valid = false;
  h->signatures_stale();   // the bands change: signatures of an earlier teb_amd_compute_h_signatures call are stale
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->ev1.e, h->stream));
  h->timed = true;
  return TEB_AMD_OK;
}

}  // namespace

extern "C" {

int teb_amd_abi_version(void) { return TEB_AMD_ABI_VERSION; }
const char* teb_amd_last_error(void) { return g_last_error.c_str(); }
int teb_amd_sizeof_config(void) { return (int)sizeof(teb_amd_config_t); }
int teb_amd_sizeof_obstacles(void) { return (int)sizeof(teb_amd_obstacles_t); }
int teb_amd_sizeof_teb_batch(void) { return (int)sizeof(teb_amd_teb_batch_t); }
int teb_amd_sizeof_results(void) { return (int)sizeof(teb_amd_results_t); }
int teb_amd_sizeof_options(void) { return (int)sizeof(teb_amd_options_t); }

void teb_amd_config_default(teb_amd_config_t* c) {   // TebConfig::TebConfig(), reference teb_config.h:245-390
  std::memset(c, 0, sizeof(*c));
  c->teb_autosize = 1; c->dt_ref = 0.3; c->dt_hysteresis = 0.1; c->min_samples = 3; c->max_samples = 500;
  c->exact_arc_length = 0; c->via_points_ordered = 0;
  c->max_vel_x = 0.4; c->max_vel_x_backwards = 0.2; c->max_vel_y = 0.0; c->max_vel_trans = 0.0; c->max_vel_theta = 0.3;
  c->acc_lim_x = 0.5; c->acc_lim_y = 0.5; c->acc_lim_theta = 0.5; c->min_turning_radius = 0;
  c->min_obstacle_dist = 0.5; c->inflation_dist = 0.6; c->dynamic_obstacle_inflation_dist = 0.6;
  c->include_dynamic_obstacles = 1; c->obstacle_poses_affected = 25; c->legacy_obstacle_association = 0;
  c->obstacle_association_force_inclusion_factor = 1.5; c->obstacle_association_cutoff_factor = 5;
  c->obstacle_proximity_ratio_max_vel = 1; c->obstacle_proximity_lower_bound = 0; c->obstacle_proximity_upper_bound = 0.5;
  c->no_inner_iterations = 5; c->no_outer_iterations = 4; c->optimization_activate = 1; c->penalty_epsilon = 0.05;
  c->weight_max_vel_x = 2; c->weight_max_vel_y = 2; c->weight_max_vel_theta = 1; c->weight_acc_lim_x = 1;
  c->weight_acc_lim_y = 1; c->weight_acc_lim_theta = 1; c->weight_kinematics_nh = 1000;
  c->weight_kinematics_forward_drive = 1; c->weight_kinematics_turning_radius = 1; c->weight_optimaltime = 1;
  c->weight_shortest_path = 0; c->weight_obstacle = 50; c->weight_inflation = 0.1; c->weight_dynamic_obstacle = 50;
  c->weight_dynamic_obstacle_inflation = 0.1; c->weight_velocity_obstacle_ratio = 0; c->weight_viapoint = 1;
  c->weight_prefer_rotdir = 50; c->weight_adapt_factor = 2.0; c->obstacle_cost_exponent = 1.0;
  c->selection_cost_hysteresis = 1.0; c->selection_prefer_initial_plan = 0.95; c->selection_obst_cost_scale = 100.0;
  c->selection_viapoint_cost_scale = 1.0; c->selection_alternative_time_cost = 0;
  c->divergence_detection_enable = 0; c->divergence_detection_max_chi_squared = 10;
  c->footprint_type = TEB_AMD_FOOTPRINT_POINT;
  c->jacobian_mode = TEB_AMD_JACOBIAN_ANALYTIC;
}

void teb_amd_options_default(teb_amd_options_t* o) {
  if (!o) return;
  std::memset(o, 0, sizeof(*o));
  o->struct_size = (int32_t)sizeof(*o);
}

int teb_amd_create(const teb_amd_config_t* cfg, int32_t max_tebs, int32_t max_poses, int32_t max_obstacles,
                   int32_t max_obstacle_vertices, int32_t max_via_points, int32_t device, void* stream,
                   teb_amd_handle_t** out) {
  return teb_amd_create_ex(cfg, max_tebs, max_poses, max_obstacles, max_obstacle_vertices, max_via_points, device, stream, nullptr, out);
}

int teb_amd_create_ex(const teb_amd_config_t* cfg, int32_t max_tebs, int32_t max_poses, int32_t max_obstacles,
                      int32_t max_obstacle_vertices, int32_t max_via_points, int32_t device, void* stream,
                      const teb_amd_options_t* options, teb_amd_handle_t** out) {
  teb_amd_options_t opt;
  teb_amd_options_default(&opt);
  if (options) {   // copy what the caller's (possibly older, shorter) struct holds
    const size_t have = options->struct_size > 0 ? (size_t)options->struct_size : sizeof(opt);
    std::memcpy(&opt, options, std::min(have, sizeof(opt)));
    opt.struct_size = (int32_t)sizeof(opt);
    if (opt.layout < TEB_AMD_LAYOUT_AUTO || opt.layout > TEB_AMD_LAYOUT_BAND_HBM || opt.hsig3d_kernel < 0 || opt.hsig3d_kernel > TEB_AMD_HSIG3D_SMALL)
      return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_options_t: unknown layout / hsig3d_kernel");
  }
  if (!cfg || !out || max_tebs <= 0 || max_poses < 2 || max_obstacles < 0 || max_obstacle_vertices < 0 || max_via_points < 0)
    return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_create: bad arguments");
  int rc = validate_config(cfg);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(TEB_AMD_ERR_NO_DEVICE, "no HIP device visible (libteb_amd has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(TEB_AMD_ERR_INVALID_ARG, "device ordinal out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(TEB_AMD_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  HIPCHK(hipSetDevice(device));
  // the kernel also owns a little static LDS (__syncthreads_or scratch): keep 1 KiB of head-room
  const size_t lds_limit = (size_t)prop.sharedMemPerBlock - kLdsHeadroomBytes;
  static_assert(TEB_AMD_MAX_POSES <= kThreads * 4, "TEB_AMD_MAX_POSES of include/teb_amd.h exceeds four poses per lane");
  const CreateLayout made = layout_at_create(max_poses, max_obstacles, lds_limit, opt.layout, kThreads, kPoseIterBandHbm, plan_bytes_of(lds_limit));
  if (made.refused == CreateLayout::BLOCKS_TOO_LARGE) return fail(TEB_AMD_ERR_CAPACITY, "TEB_AMD_LAYOUT_BLOCKS_LDS: max_poses too large for the block layout");
  if (made.refused == CreateLayout::CAPACITY) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "max_poses=%d needs %zu B of LDS per workgroup (device limit %zu B, thread limit %d poses)",
                  max_poses, made.lds, lds_limit, made.thread_limit);
    return fail(TEB_AMD_ERR_CAPACITY, buf);
  }
  const int solver = made.layout;
  const size_t assoc_bytes = sizeof(int) * (size_t)max_tebs * max_poses * (size_t)(max_obstacles > 0 ? max_obstacles : 1);
  if (assoc_bytes > ((size_t)64 << 30)) return fail(TEB_AMD_ERR_CAPACITY, "association table would exceed 64 GiB");

  teb_amd_handle* h = new teb_amd_handle();
  h->device = device;
  h->cfg = *cfg;
  h->opt = opt;
  h->max_tebs = max_tebs; h->stride = max_poses; h->max_obst = max_obstacles; h->max_verts = max_obstacle_vertices;
  h->max_via = max_via_points;
  h->layout.solver = solver; h->solver_created = solver;
  h->lds_limit = lds_limit;
  h->num_cus = prop.multiProcessorCount;
  h->layout.plan = make_lds_plan(max_poses, solver, 0, h->lds_limit);
  // per-band HBM buffer: the copy of H for rejected trials (SOLVER_CR, banded LDL^T) or the blocks the cyclic reduction of a
  // SOLVER_BAND handle works on (D, L, f: nb * (2 * kBlk + 8) doubles)
  h->hmat_stride = std::max(hbm_scratch_doubles(max_poses, SOLVER_BAND), hbm_scratch_doubles(max_poses, solver));   // every layout may be launched
  h->hmat_stride = (h->hmat_stride + 1) & ~(size_t)1;   // every band's slice 16-byte aligned (the multi-CU mode writes it with 16-byte stores)
  h->band_ldlt = opt.band_ldlt != 0;
  if (solver == SOLVER_BANDG) h->band_ldlt = 0;   // the sequential LDL^T works in place on an LDS band only
  if (stream) h->stream = reinterpret_cast<hipStream_t>(stream);
  else {
    if (hipStreamCreateWithFlags(&h->own_stream.s, hipStreamNonBlocking) != hipSuccess) { delete h; return fail(TEB_AMD_ERR_HIP, "hipStreamCreate failed"); }
    h->stream = h->own_stream.s;
  }
  const size_t BS = (size_t)max_tebs * max_poses;
  const size_t Mo = max_obstacles > 0 ? max_obstacles : 1;
  AllocRun A;
  if (!h->scene.alloc(Mo, 1, max_obstacle_vertices, max_via_points, 0)) A(hipErrorOutOfMemory);
  A(h->bands.alloc(max_tebs, max_poses)); A(h->snap.alloc(max_tebs, max_poses));
  A(h->assoc_cnt.alloc(BS)); A(h->assoc.alloc(BS * Mo)); A(h->assoc_ovf.alloc(max_tebs)); A(h->legacy_idx.alloc((size_t)max_tebs * Mo));
  A(h->via_pose.alloc((size_t)max_tebs * (max_via_points > 0 ? max_via_points : 1)));
  A(h->Hbackup.alloc((size_t)max_tebs * h->hmat_stride));
  A(h->clk.alloc(4));
  h->hband_stride = solver == SOLVER_BANDG ? (((size_t)hbo(4 * max_poses) + 2 + 1) & ~(size_t)1) : 0;   // even: the bands' slices are zeroed in 16-byte stores
  A(h->Hband.alloc((size_t)max_tebs * h->hband_stride));
  A(h->dbg_H.alloc((size_t)4 * max_poses * kBand)); A(h->dbg_b.alloc((size_t)4 * max_poses)); A(h->dbg_chi2.alloc(4));
  A(h->sel_cost.alloc(2)); A(h->sel_idx.alloc(1)); A(h->err_flag.alloc(1));
  A(h->pack_dev.alloc(kPackMaxDoubles));
  if (A.ok() && hipHostMalloc(reinterpret_cast<void**>(&h->pack_host.p), kPackMaxDoubles * sizeof(double), hipHostMallocDefault) != hipSuccess) h->pack_host.p = nullptr;   // (optional: without it the strided copies are used)
  A(h->stage_x.alloc((size_t)max_poses + 2)); A(h->stage_y.alloc((size_t)max_poses + 2)); A(h->stage_yaw.alloc((size_t)max_poses + 2));
  A(h->out_cmd.alloc(4 * (size_t)max_tebs)); A(h->out_prof.alloc((size_t)max_tebs * (max_poses + 1) * 3)); A(h->out_traj.alloc(BS * 7));
  A(h->hsig.alloc((size_t)max_tebs * (Mo > 2 ? Mo : 2))); A(h->hs_pre.alloc(Mo)); A(h->hs_pim.alloc(Mo)); A(h->hs_pex.alloc(Mo));
  if (A.ok()) A(hipEventCreate(&h->ev0.e));
  if (A.ok()) A(hipEventCreate(&h->ev1.e));
  // every instantiation of the build may be launched (teb_amd_set_obstacles / per-launch choice) with any plan up to the limit
#define TEB_OPT_FULL_LDS(S, J, P) \
  if (const void* k = TEB_OPT_KERNEL_FN(S, J, P)()) if (A.ok()) A(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_limit));
  TEB_OPT_FOR_ALL(TEB_OPT_FULL_LDS)
#undef TEB_OPT_FULL_LDS
  if (A.ok()) A(h->bands.zero_at_create([](void* p, size_t bytes) { return hipMemset(p, 0, bytes); }));
  if (!A.ok()) { delete h; return fail(TEB_AMD_ERR_HIP, "device allocation / kernel attribute setup failed"); }
  *out = h;
  return TEB_AMD_OK;
}

// (the order of the teardown: ~teb_amd_handle)
void teb_amd_destroy(teb_amd_handle_t* h) { delete h; }

namespace {
// The distance path and the layout of the tables of a scene store, for an obstacle cache of lay.max_cache entries (layout_per_table), and
// what the answer needs: the HBM band buffer of a handle that was created without one, the LDS plan.
int choose_scene_layout(teb_amd_handle* h, bool pointlike_rows, const ClassList& cl, SceneLayout& lay) {
  const TableLayout t = fleet_layout_per_table(pointlike_rows, cl.cfgs, cl.n, h->opt.generic_distance_path != 0, h->solver_created, h->opt.layout,
                                               lay.max_cache, h->stride, h->lds_limit, plan_bytes_of(h->lds_limit));
  if (t.hbm_band && h->hband_stride == 0) {
    h->hband_stride = ((size_t)hbo(4 * h->stride) + 2 + 1) & ~(size_t)1;
    HIPCHK(h->Hband.alloc((size_t)h->max_tebs * h->hband_stride));
  }
  lay.solver = t.layout;
  lay.fast_points = t.fast_points;
  lay.plan = make_lds_plan(h->stride, t.layout, t.cache_entries, h->lds_limit);
  return TEB_AMD_OK;
}
// (Re)derives everything that depends on BOTH obstacle tables and the configuration, for the ns tables `tabs` - table s under the
// configuration cl.of_scene(s), the distance path over every class of cl (teb_fleet_host.hpp) - whose rows `store` holds
// one after the other (scene_segments; ONE table for the single scene of the handle): the lists AddEdgesObstacles /
// AddEdgesDynamicObstacles visit and the obstacles in cache order, uploaded; the SceneDev of every table - each points at its own
// segment with indices local to it, so the kernel's arithmetic is the single-scene one - into `scenes` and, for a fleet launch to index,
// into `scenes_dev`; the distance path (point-like LDS cache, sized for the largest table, or generic) and the layout that goes with it
// into `lay`; the static list of table 0 into `first_static`. Nothing is touched when the layout cannot be had.
int commit_tables(teb_amd_handle* h, const ClassList& cl, const HostObst* tabs, const int* via_count, size_t ns, DevSceneStore& store, SceneLayout& lay,
                  std::vector<SceneDev>& scenes, DevBuf<SceneDev>* scenes_dev, std::vector<int>* first_static) {
  const std::vector<SceneSegment> seg = scene_segments(tabs, via_count, ns);
  SceneLists all, d;   // all: the lists of every table at its segment
  SceneLayout chosen;
  std::vector<int> st0;
  bool pointlike = true;
  scenes.assign(ns, SceneDev{});
  for (size_t s = 0; s < ns; ++s) {
    const size_t M = tabs[s].rows();
    derive_scene_lists(cl.of_scene(s), tabs[s], d);
    all.st.resize(seg[s].row + M, 0); all.dy.resize(seg[s].row + M, 0);
    std::copy(d.st.begin(), d.st.end(), all.st.begin() + seg[s].row);
    std::copy(d.dy.begin(), d.dy.end(), all.dy.begin() + seg[s].row);
    all.lo.insert(all.lo.end(), d.lo.begin(), d.lo.end());   // 5 M values: planes of stride M from seg[s].list on
    pointlike = pointlike && d.pointlike_rows;
    chosen.max_cache = std::max(chosen.max_cache, (int)M);
    scenes[s] = store.view(seg[s], (int)M, via_count[s], (int)d.st.size(), (int)d.dy.size(), d.static_radius_zero, 0);
    if (s == 0) st0 = d.st;
  }
  if (int rc = choose_scene_layout(h, pointlike, cl, chosen)) return rc;
  for (auto& q : scenes) q.fast_points = chosen.fast_points;   // one distance path for the whole launch
  HIPCHK(store.upload_lists(h->stream, all));
  if (scenes_dev) HIPCHK(hipMemcpyAsync(scenes_dev->p, scenes.data(), ns * sizeof(SceneDev), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // host vectors go out of scope
  lay = chosen;
  if (first_static) *first_static = std::move(st0);
  return TEB_AMD_OK;
}
// the single scene: the table held in h->hob
int commit_obstacles(teb_amd_handle* h) {
  std::vector<SceneDev> one;
  if (int rc = commit_tables(h, own_class(h), &h->hob, &h->nvia, 1, h->scene, h->layout, one, nullptr, &h->host_static)) return rc;
  h->static_radius_zero = one[0].static_radius_zero; h->n_static = one[0].n_static; h->n_dyn = one[0].n_dyn;
  h->signatures_stale();   // signatures depend on the obstacle table and on include_dynamic_obstacles
  return TEB_AMD_OK;
}
// fleet mode: the tables of the scene set, and the SceneDev array a fleet launch indexes
int commit_fleet(teb_amd_handle* h) {
  auto& F = h->fleet;
  std::vector<SceneDev> views;
  F.sigs.clear(); F.hs_prod_valid = false;   // signatures depend on the tables of the set and on include_dynamic_obstacles
  return commit_tables(h, fleet_classes(h), F.tabs.data(), F.via_count.data(), F.tabs.size(), F.store, F.layout, views, &F.scenes, nullptr);
}
// both, as far as they hold anything (teb_amd_set_config)
int commit_all(teb_amd_handle* h) {
  int rc = h->M > 0 ? commit_obstacles(h) : TEB_AMD_OK;
  if (!rc && h->fleet.n_scenes > 0 && h->fleet.classes.empty()) rc = commit_fleet(h);   // (with a class map the set's lists follow the classes)
  return rc;
}

// the calls that read or write THE scene of the handle are not available while a scene set is installed (teb_amd.h, fleet batches)
int refuse_in_fleet_mode(const teb_amd_handle* h, const char* call) {
  if (h->fleet.n_scenes > 0)
    return fail(TEB_AMD_ERR_INVALID_ARG, std::string(call) + ": not available while scenes are set (fleet mode); call teb_amd_clear_scenes first");
  return TEB_AMD_OK;
}
// ... and the per-scene calls need one
int require_fleet_mode(const teb_amd_handle* h, const char* call) {
  if (h->fleet.n_scenes <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(call) + ": no scenes set (teb_amd_set_scenes)");
  return TEB_AMD_OK;
}
// every band < B maps to a scene of the set (the check of teb_amd_optimize_batch)
int check_band_scenes(const teb_amd_handle* h, int B) {
  const auto& F = h->fleet;
  for (int b = 0; b < B; ++b)
    if (F.band_scene[b] >= F.n_scenes) {
      char buf[160];
      std::snprintf(buf, sizeof buf, "band %d maps to scene %d, but %d scenes are set (teb_amd_set_band_scenes)", b, F.band_scene[b], F.n_scenes);
      return fail(TEB_AMD_ERR_INVALID_ARG, buf);
    }
  return TEB_AMD_OK;
}
// The planners of a scene set and their first B bands (BandGroups of teb_hcp_host.hpp), one group per scene. The single scene's one
// planner is BandGroups(1, B, nullptr).
int scene_groups(const teb_amd_handle* h, int B, BandGroups& G) {
  if (int rc = check_band_scenes(h, B)) return rc;
  G = BandGroups(h->fleet.n_scenes, B, h->fleet.band_scene.data());
  return TEB_AMD_OK;
}
// best[s] is a band of scene s or negative (best NULL: none)
int check_best_per_scene(const BandGroups& G, const int32_t* best, const char* call) {
  for (int s = 0; best && s < G.size(); ++s)
    if (best[s] >= 0 && !G.has(s, best[s])) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "%s: best[%d] = %d is not a band of scene %d", call, s, best[s], s);
      return fail(TEB_AMD_ERR_INVALID_ARG, buf);
    }
  return TEB_AMD_OK;
}
}  // namespace

namespace { int upload_class_table(teb_amd_handle* h); }   // (fleet batches, below)

int teb_amd_set_config(teb_amd_handle_t* h, const teb_amd_config_t* cfg) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!cfg) return fail(TEB_AMD_ERR_INVALID_ARG, "null config");
  rc = validate_config(cfg);
  if (rc) return rc;   // the handle keeps its previous configuration
  const bool lists_changed = (cfg->include_dynamic_obstacles != h->cfg.include_dynamic_obstacles) ||
                             (cfg->footprint_type != h->cfg.footprint_type);
  const teb_amd_config_t previous = h->cfg;
  h->cfg = *cfg;
  // derives the static / dynamic lists, the distance path and the LDS plan from h->cfg: of the single scene and of every scene of a set
  if (lists_changed && (rc = commit_all(h))) {   // "keeps its previous configuration" (teb_amd.h): put it back together with what is derived from it
    const std::string why = g_last_error;
    h->cfg = previous;
    (void)commit_all(h);
    return fail(rc, why);
  }
  h->consumers_valid = false;
  // a fleet without a class map launches under the handle's configuration as its one class (with a map the table is the map's)
  return h->fleet.classes.empty() && std::memcmp(&previous, cfg, sizeof previous) != 0 ? upload_class_table(h) : TEB_AMD_OK;
}

namespace {
// Uploads the rows of t to the device table of the single scene from row `first` on (voff: first .. first + M) and its vertices from 0 on.
int upload_obstacle_rows(teb_amd_handle* h, const HostObst& t, size_t first) {
  HIPCHK(h->scene.upload_rows(h->stream, t, first, first, 0));
  HIPCHK(hipStreamSynchronize(h->stream));   // the uploads read `t`
  return TEB_AMD_OK;
}

// The device rows hold table t: the host copy takes it over and everything derived from the table is derived again.
int install_obstacles(teb_amd_handle* h, HostObst&& t) {
  h->M = (int)t.rows();
  h->hs_prod_valid = false;
  h->hob = std::move(t);
  return commit_obstacles(h);
}
}  // namespace

int teb_amd_set_obstacles(teb_amd_handle_t* h, const teb_amd_obstacles_t* o) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_set_obstacles"))) return rc;
  if (!o || o->count < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "null obstacle table");
  if (o->count > h->max_obst) return fail(TEB_AMD_ERR_CAPACITY, "more obstacles than max_obstacles");
  HostObst t;
  if (const char* bad = parse_obstacle_table(o, t)) return fail(TEB_AMD_ERR_INVALID_ARG, bad);
  if ((int)t.pvx.size() > h->max_verts) return fail(TEB_AMD_ERR_CAPACITY, "more polygon vertices than max_obstacle_vertices");
  rc = upload_obstacle_rows(h, t, 0);
  if (rc) return rc;
  return install_obstacles(h, std::move(t));
}

int teb_amd_set_via_points(teb_amd_handle_t* h, int32_t count, const double* x, const double* y) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_set_via_points"))) return rc;
  if (count < 0 || (count > 0 && (!x || !y))) return fail(TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays");
  if (count > h->max_via) return fail(TEB_AMD_ERR_CAPACITY, "more via-points than max_via_points");
  if (count > 0) {
    HIPCHK(h->scene.upload_vias(h->stream, x, y, (size_t)count));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  h->nvia = count;
  return TEB_AMD_OK;
}

// ---- fleet batches (teb_amd.h): a set of scenes and a band -> scene map ---------------------------------------------------------------
namespace {
constexpr size_t kFleetPad = 8;   // elements past every buffer of the scene set's store: the segment of an empty scene at the very end still points at storage
// THE install of the class table a fleet launch reads: the classes of the map and the class of every scene, or - without a map - one
// class, the handle's configuration, and a class array of zeros. Every change of either goes through here; nothing else writes the two
// buffers. Before the fleet storage exists there is nothing to write (fleet_allocate comes through here).
int upload_class_table(teb_amd_handle* h) {
  auto& F = h->fleet;
  if (!F.class_of_scene.p) return TEB_AMD_OK;
  const ClassList cl = fleet_classes(h);
  std::vector<int> of((size_t)h->max_tebs, 0);
  if (cl.class_of) std::copy(F.class_of.begin(), F.class_of.end(), of.begin());   // (n_scenes <= max_tebs)
  HIPCHK(ensure(F.cfgs, (size_t)cl.n));
  HIPCHK(hipMemcpyAsync(F.cfgs.p, cl.cfgs, (size_t)cl.n * sizeof(teb_amd_config_t), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(F.class_of_scene.p, of.data(), of.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // `of` goes out of scope, the caller may change its configurations
  h->consumers_valid = false;   // the consumers read the class of a band's scene
  return TEB_AMD_OK;
}
// the map has the lifetime of the scene count: forgotten where the planners of the scenes are (new_planners)
int forget_classes(teb_amd_handle* h) {
  auto& F = h->fleet;
  if (F.classes.empty()) return TEB_AMD_OK;
  F.classes.clear(); F.class_of.clear();
  return upload_class_table(h);
}
int fleet_allocate(teb_amd_handle* h) {
  auto& F = h->fleet;
  if (F.allocated) return TEB_AMD_OK;
  const size_t T = (size_t)h->max_tebs;
  // (every scene has one first-vertex offset more than rows, and there are at most T scenes)
  AllocRun A;
  if (!F.store.alloc((size_t)std::max(h->max_obst, 0), T, (size_t)std::max(h->max_verts, 0), (size_t)std::max(h->max_via, 0), kFleetPad)) A(hipErrorOutOfMemory);
  A(F.scenes.alloc(T)); A(F.scene_of.alloc(T)); A(F.cfgs.alloc(1)); A(F.class_of_scene.alloc(T)); A(F.sel_last.alloc(T)); A(F.sel_init.alloc(T)); A(F.sel_idx.alloc(T)); A(F.sel_cost.alloc(T));
  const size_t rows = (size_t)std::max(h->max_obst, 0) + kFleetPad;   // one product per row of the set's store
  A(F.hs_pre.alloc(rows)); A(F.hs_pim.alloc(rows)); A(F.hs_pex.alloc(rows)); A(F.hs_off.alloc(T + 1));
#ifdef TEB_AMD_HAS_FLEET_UNITS
#define TEB_FLEET_FULL_LDS(S, P) \
  if (const void* k = TEB_FLEET_KERNEL_FN(S, P)()) if (A.ok()) A(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->lds_limit));
  TEB_FLEET_FOR_ALL(TEB_FLEET_FULL_LDS)
#undef TEB_FLEET_FULL_LDS
#endif
  if (F.band_scene.empty()) F.band_scene.assign(T, 0);
  if (A.ok()) A(hipMemcpy(F.scene_of.p, F.band_scene.data(), T * sizeof(int), hipMemcpyHostToDevice));
  if (!A.ok()) {
    (void)hipGetLastError();
    F.release();
    return fail(TEB_AMD_ERR_HIP, "teb_amd_set_scenes: device allocation of the fleet storage failed");
  }
  F.allocated = true;
  if (int rc = upload_class_table(h)) { F.release(); return rc; }
  return TEB_AMD_OK;
}
// The tail of teb_amd_set_scenes and teb_amd_set_scenes_from_costmaps: the host tables of the n scenes exist and fit the capacities of the
// handle; vias = sum of vc, in via_x / via_y one scene after the other.
int install_scene_set(teb_amd_handle* h, std::vector<HostObst>&& tabs, std::vector<int>&& vc, const double* via_x, const double* via_y, size_t vias) {
  const int n_scenes = (int)tabs.size();
  int rc = fleet_allocate(h);
  if (rc) return rc;
  auto& F = h->fleet;
  // rows, vertices and via-points of the scenes one after the other (voff: M + 1 entries per scene, local to the scene's vertices)
  HostObst all;
  for (const HostObst& t : tabs) all.append_segment(t);
  // From here on the rows of the previous set are overwritten in place: whatever fails now is a HIP error, and the handle is then left
  // in single-scene mode (n_scenes = 0) - nothing else consistent is left to return to.
  hipError_t e = hipSuccess;
  auto U = [&](hipError_t r) { if (e == hipSuccess) e = r; };
  U(F.store.upload_rows(h->stream, all, 0, 0, 0));
  U(F.store.upload_vias(h->stream, via_x, via_y, vias));
  U(hipStreamSynchronize(h->stream));   // the uploads read `all` and the caller's arrays
  if (e != hipSuccess) {
    F.n_scenes = 0; F.tabs.clear(); F.via_count.clear(); F.new_planners(0); (void)forget_classes(h);
    return fail(TEB_AMD_ERR_HIP, std::string("teb_amd_set_scenes: upload of the scene set -> ") + hipGetErrorString(e));
  }
  F.tabs = std::move(tabs);
  F.via_count = std::move(vc);
  if (F.class_of.size() != (size_t)n_scenes && (rc = forget_classes(h))) { F.n_scenes = 0; F.tabs.clear(); F.via_count.clear(); F.new_planners(0); return rc; }   // the class map belongs to the scene count, like the planners below
  rc = commit_fleet(h);   // (the lists of every scene from its class)
  if (rc) { F.n_scenes = 0; F.tabs.clear(); F.via_count.clear(); F.new_planners(0); (void)forget_classes(h); return rc; }
  F.n_scenes = n_scenes;
  if (F.memory.size() != (size_t)n_scenes) F.new_planners(n_scenes);   // a remembered class belongs to a robot: kept while the fleet keeps its size
  return TEB_AMD_OK;
}
// what the tables and via-points of a scene set may hold together (parse_scene_inputs, teb_costmap_host.hpp)
extern "C++" SceneCaps handle_caps(const teb_amd_handle* h) { return SceneCaps{(size_t)h->max_obst, (size_t)h->max_verts, (size_t)h->max_via}; }
}  // namespace

int teb_amd_set_scenes(teb_amd_handle_t* h, int32_t n_scenes, const teb_amd_obstacles_t* obstacles, const int32_t* via_count, const double* via_x,
                       const double* via_y) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_scenes < 1 || !obstacles) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_scenes: needs at least one scene");
  if (n_scenes > h->max_tebs) return fail(TEB_AMD_ERR_CAPACITY, "more scenes than max_tebs");
  // everything is parsed and checked before the first upload: on an error the previous scene set stays installed
  SceneInputs in;
  if (Refusal r = parse_scene_inputs(n_scenes, obstacles, "null obstacle table", via_count, via_x, via_y, handle_caps(h), in)) return fail(r.code, r.text);
  return install_scene_set(h, std::move(in.tabs), std::move(in.vc), via_x, via_y, in.vias);
}

int teb_amd_set_band_scenes(teb_amd_handle_t* h, const int32_t* scene_of, int32_t count) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (count < 0 || (count > 0 && !scene_of)) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_band_scenes: bad arguments");
  if (count > h->max_tebs) return fail(TEB_AMD_ERR_CAPACITY, "more bands than max_tebs");
  for (int b = 0; b < count; ++b)
    if (scene_of[b] < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_band_scenes: negative scene index");
  auto& F = h->fleet;
  F.band_scene.assign((size_t)h->max_tebs, 0);   // bands >= count: scene 0
  F.sigs.clear();   // per-scene signatures were computed against the previous map
  h->consumers_valid = false;   // with a class map the consumers read the class of a band's scene
  std::copy(scene_of, scene_of + count, F.band_scene.begin());
  if (F.allocated) {
    HIPCHK(hipMemcpyAsync(F.scene_of.p, F.band_scene.data(), F.band_scene.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return TEB_AMD_OK;
}

int teb_amd_get_band_scenes(teb_amd_handle_t* h, int32_t* scene_of, int32_t capacity, int32_t* count) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (count) *count = h->B;
  if (!scene_of) return TEB_AMD_OK;
  if (capacity < h->B) return fail(TEB_AMD_ERR_CAPACITY, "teb_amd_get_band_scenes: more bands than capacity");
  for (int b = 0; b < h->B; ++b) scene_of[b] = (size_t)b < h->fleet.band_scene.size() ? h->fleet.band_scene[b] : 0;
  return TEB_AMD_OK;
}

int teb_amd_clear_scenes(teb_amd_handle_t* h) {
  int rc = check_handle(h);
  if (rc) return rc;
  h->fleet.n_scenes = 0;   // the single-scene table, its lists and its layout are as they were
  h->fleet.tabs.clear(); h->fleet.via_count.clear();
  h->fleet.sigs.clear(); h->fleet.hs_prod_valid = false;
  h->fleet.new_planners(0);
  return forget_classes(h);
}

int teb_amd_get_scene_count(teb_amd_handle_t* h, int32_t* n_scenes) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!n_scenes) return fail(TEB_AMD_ERR_INVALID_ARG, "null output");
  *n_scenes = h->fleet.n_scenes;
  return TEB_AMD_OK;
}

int teb_amd_set_scene_configs(teb_amd_handle_t* h, int32_t n_classes, const teb_amd_config_t* configs, int32_t n_scenes, const int32_t* class_of_scene) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_set_scene_configs"))) return rc;
  auto& F = h->fleet;
  if (n_classes < 1 || !configs || !class_of_scene) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_scene_configs: needs at least one class and a class for every scene");
  char buf[256];
  if (n_scenes != F.n_scenes) {
    std::snprintf(buf, sizeof buf, "teb_amd_set_scene_configs: n_scenes = %d, but %d scenes are set", n_scenes, F.n_scenes);
    return fail(TEB_AMD_ERR_INVALID_ARG, buf);
  }
  // everything is checked before anything live is touched
  for (int k = 0; k < n_classes; ++k)
    if ((rc = validate_config(configs + k))) {
      std::snprintf(buf, sizeof buf, "teb_amd_set_scene_configs: class %d: %s", k, g_last_error.c_str());
      return fail(rc, buf);
    }
  if (const ClassRefusal r = fleet_classes_agree(configs, n_classes); !r.ok()) {
    std::snprintf(buf, sizeof buf, "teb_amd_set_scene_configs: class %d: %s %s", r.cls, r.field, r.why);
    return fail(TEB_AMD_ERR_INVALID_ARG, buf);
  }
  if (const int s = first_scene_without_class(class_of_scene, n_scenes, n_classes); s >= 0) {
    std::snprintf(buf, sizeof buf, "teb_amd_set_scene_configs: class_of_scene[%d] = %d is not one of the %d classes", s, class_of_scene[s], n_classes);
    return fail(TEB_AMD_ERR_INVALID_ARG, buf);
  }
  // the lists of every scene, the distance path and the layout under the new classes; a layout that cannot be had leaves nothing touched
  // (commit_tables), anything later puts the previous map - or none - back together with what is derived from it
  std::vector<teb_amd_config_t> prev_classes(configs, configs + n_classes);
  std::vector<int> prev_of(class_of_scene, class_of_scene + n_scenes);
  F.classes.swap(prev_classes); F.class_of.swap(prev_of);
  if ((rc = commit_fleet(h)) || (rc = upload_class_table(h))) {
    const std::string why = g_last_error;
    F.classes.swap(prev_classes); F.class_of.swap(prev_of);
    (void)commit_fleet(h);
    (void)upload_class_table(h);
    return fail(rc, why);
  }
  return TEB_AMD_OK;
}

int teb_amd_clear_scene_configs(teb_amd_handle_t* h) {
  int rc = check_handle(h);
  if (rc) return rc;
  auto& F = h->fleet;
  if (F.classes.empty()) return TEB_AMD_OK;
  std::vector<teb_amd_config_t> prev_classes;
  std::vector<int> prev_of;
  F.classes.swap(prev_classes); F.class_of.swap(prev_of);
  if ((F.n_scenes > 0 && (rc = commit_fleet(h))) || (rc = upload_class_table(h))) {   // the handle's footprint may not fit the layout: the map stays
    const std::string why = g_last_error;
    F.classes.swap(prev_classes); F.class_of.swap(prev_of);
    if (F.n_scenes > 0) (void)commit_fleet(h);
    (void)upload_class_table(h);
    return fail(rc, why);
  }
  return TEB_AMD_OK;
}

int teb_amd_get_scene_configs(teb_amd_handle_t* h, int32_t* n_classes, int32_t* class_of_scene, int32_t capacity) {
  int rc = check_handle(h);
  if (rc) return rc;
  const auto& F = h->fleet;
  if (n_classes) *n_classes = (int32_t)F.classes.size();
  if (!class_of_scene || F.classes.empty()) return TEB_AMD_OK;
  if (capacity < (int32_t)F.class_of.size()) return fail(TEB_AMD_ERR_CAPACITY, "teb_amd_get_scene_configs: more scenes than capacity");
  std::copy(F.class_of.begin(), F.class_of.end(), class_of_scene);
  return TEB_AMD_OK;
}

int teb_amd_select_best_per_scene(teb_amd_handle_t* h, const int32_t* last_best, const int32_t* initial_plan, int32_t* best, double* best_cost) {
  int rc = check_handle(h);
  if (rc) return rc;
  auto& F = h->fleet;
  if (F.n_scenes <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_select_best_per_scene: no scenes set (teb_amd_set_scenes)");
  if (!best) return fail(TEB_AMD_ERR_INVALID_ARG, "null output");
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs uploaded");
  const int ns = F.n_scenes;
  std::vector<int> lb(ns, -1), ip(ns, -1);
  for (int s = 0; s < ns; ++s) {
    if (last_best && last_best[s] < h->B) lb[s] = last_best[s];
    if (initial_plan && initial_plan[s] < h->B) ip[s] = initial_plan[s];
  }
  HIPCHK(hipMemcpyAsync(F.sel_last.p, lb.data(), ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(F.sel_init.p, ip.data(), ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
  LAUNCH(select_best_per_scene_kernel, dim3(ns), dim3(kThreads), 0, h->stream, h->bands.cost.p, F.scene_of.p, h->B, F.sel_last.p, F.sel_init.p,
         F.cfgs.p, F.class_of_scene.p, F.sel_cost.p, F.sel_idx.p);
  std::vector<double> cst(ns);
  HIPCHK(hipMemcpyAsync(best, F.sel_idx.p, ns * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(cst.data(), F.sel_cost.p, ns * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // (lb / ip / cst are read and written until here)
  if (best_cost) std::copy(cst.begin(), cst.end(), best_cost);
  return TEB_AMD_OK;
}

int teb_amd_upload_tebs(teb_amd_handle_t* h, const teb_amd_teb_batch_t* bt) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!bt || bt->count <= 0 || !bt->n || !bt->x || !bt->y || !bt->theta || !bt->dt)
    return fail(TEB_AMD_ERR_INVALID_ARG, "bad TEB batch");
  if (bt->count > h->max_tebs) return fail(TEB_AMD_ERR_CAPACITY, "more TEBs than max_tebs");
  const int B = bt->count;
  int nmax = 0;
  for (int b = 0; b < B; ++b) {
    if (bt->n[b] < 2) return fail(TEB_AMD_ERR_INVALID_ARG, "a TEB needs at least 2 poses");
    if (bt->n[b] > bt->stride) return fail(TEB_AMD_ERR_INVALID_ARG, "n[b] > stride");
    nmax = bt->n[b] > nmax ? bt->n[b] : nmax;
  }
  if (nmax > h->stride) return fail(TEB_AMD_ERR_CAPACITY, "a TEB has more poses than max_poses");
  const int wc_pack = bt->stride < h->stride ? bt->stride : h->stride;   // whole rows, like the strided copies: the padding stays the caller's
  const UploadMsg msg{(size_t)B, (size_t)wc_pack};
  if (h->pack_host.p && msg.size() <= kPackMaxDoubles) {   // small batch: one packed message, one copy, one kernel
    const int wc = wc_pack;
    const size_t plane = msg.plane();
    pack_upload(*bt, msg.w, h->pack_host.p);
    HIPCHK(hipMemcpyAsync(h->pack_dev.p, h->pack_host.p, msg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const int grid = (int)std::min<size_t>(256, (std::max<size_t>(plane, 3 * (size_t)B) + 255) / 256);
    LAUNCH(unpack_bands_kernel, dim3(grid), dim3(256), 0, h->stream, h->pack_dev.p, B, wc, h->stride, h->bands.strips.n.p, h->bands.has_vs.p, h->bands.has_vg.p, h->bands.rotdir.p,
           h->bands.via_en.p, h->bands.vs.p, h->bands.vg.p, h->bands.strips.x.p, h->bands.strips.y.p, h->bands.strips.th.p, h->bands.strips.dt.p, h->bands.optimized.p);
    HIPCHK(hipStreamSynchronize(h->stream));   // (the pinned buffer is reused by the next call)
    h->B = B;
    h->bands_changed(nmax);
    return TEB_AMD_OK;
  }
  const size_t w = (size_t)(bt->stride < h->stride ? bt->stride : h->stride) * sizeof(double);
  const size_t sp = (size_t)bt->stride * sizeof(double), dp = (size_t)h->stride * sizeof(double);
  HIPCHK(hipMemcpy2DAsync(h->bands.strips.x.p, dp, bt->x, sp, w, B, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpy2DAsync(h->bands.strips.y.p, dp, bt->y, sp, w, B, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpy2DAsync(h->bands.strips.th.p, dp, bt->theta, sp, w, B, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpy2DAsync(h->bands.strips.dt.p, dp, bt->dt, sp, w, B, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.strips.n.p, bt->n, B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  const BandAttrArrays at = attrs_of(*bt);
  HIPCHK(hipMemcpyAsync(h->bands.has_vs.p, at.has_vs.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.has_vg.p, at.has_vg.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.rotdir.p, at.rotdir.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.via_en.p, at.via_en.data(), B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.vs.p, at.vs.data(), 3 * (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.vg.p, at.vg.data(), 3 * (size_t)B * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->bands.optimized.p, 0, B * sizeof(int), h->stream));   // bands from the host: optimized_ unknown -> false
  HIPCHK(hipStreamSynchronize(h->stream));
  h->B = B;
  h->bands_changed(nmax);
  return TEB_AMD_OK;
}

int teb_amd_download_tebs(teb_amd_handle_t* h, teb_amd_teb_batch_t* bt) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!bt || !bt->n || !bt->x || !bt->y || !bt->theta || !bt->dt) return fail(TEB_AMD_ERR_INVALID_ARG, "bad TEB batch");
  if (bt->count < h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "batch too small for the resident TEBs");
  const int B = h->B;
  if (B == 0) return TEB_AMD_OK;   // an empty handle (before the first upload, after every band was dropped, a rank without candidates): nothing to copy
  {
    const int wc = bt->stride < h->stride ? bt->stride : h->stride;
    const DownloadMsg msg{(size_t)B, (size_t)wc};
    const size_t plane = msg.plane(), count = msg.size();
    if (h->pack_host.p && count <= kPackMaxDoubles) {   // small batch: one gather kernel, one copy
      const int grid = (int)std::min<size_t>(256, (plane + 255) / 256);
      LAUNCH(pack_bands_kernel, dim3(grid), dim3(256), 0, h->stream, h->pack_dev.p, B, wc, h->stride, h->bands.strips.n.p, h->bands.strips.x.p, h->bands.strips.y.p, h->bands.strips.th.p, h->bands.strips.dt.p);
      HIPCHK(hipMemcpyAsync(h->pack_host.p, h->pack_dev.p, count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
      HIPCHK(hipStreamSynchronize(h->stream));
      const double* m = h->pack_host.p;
      for (int b = 0; b < B; ++b) if ((int)m[msg.n() + b] > bt->stride) return fail(TEB_AMD_ERR_CAPACITY, "host batch stride too small for the resized TEB");
      unpack_download(m, msg.B, msg.w, *bt);
      return TEB_AMD_OK;
    }
  }
  std::vector<int> n(B);
  HIPCHK(hipMemcpyAsync(n.data(), h->bands.strips.n.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) if (n[b] > bt->stride) return fail(TEB_AMD_ERR_CAPACITY, "host batch stride too small for the resized TEB");
  const size_t w = (size_t)(bt->stride < h->stride ? bt->stride : h->stride) * sizeof(double);
  const size_t hp = (size_t)bt->stride * sizeof(double), dp = (size_t)h->stride * sizeof(double);
  HIPCHK(hipMemcpy2DAsync(bt->x, hp, h->bands.strips.x.p, dp, w, B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpy2DAsync(bt->y, hp, h->bands.strips.y.p, dp, w, B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpy2DAsync(bt->theta, hp, h->bands.strips.th.p, dp, w, B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpy2DAsync(bt->dt, hp, h->bands.strips.dt.p, dp, w, B, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) bt->n[b] = n[b];
  return TEB_AMD_OK;
}

namespace {
// teb_amd_optimize_batch (cost_mode 0 / 1: without / with the costs under the triple of the call) and teb_amd_optimize_batch_per_class
// (kCostPerClass: the triple of every band's class, read by the fleet units)
int optimize_batch(teb_amd_handle* h, int32_t inner, int32_t outer, int cost_mode, double obst_cost_scale, double viapoint_cost_scale,
                   int32_t alternative_time_cost) {
  int rc = TEB_AMD_OK;
  if (inner < 0 || outer < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "negative iteration count");
  const bool fleet = h->fleet.n_scenes > 0;
  if (fleet) {   // fleet mode (teb_amd_set_scenes): every band against its own scene, in one launch
#ifndef TEB_AMD_HAS_FLEET_UNITS
    return fail(TEB_AMD_ERR_UNSUPPORTED, "fleet launches exist in the product library only; this one is the variant built with [" TEB_AMD_VARIANT_DEFINES "]");
#else
    if (!fleet_classes_agree(fleet_classes(h).cfgs, fleet_classes(h).n).ok())   // (a map was checked at its install: this is the handle's own configuration)
      return fail(TEB_AMD_ERR_INVALID_ARG, "fleet launches need jacobian_mode TEB_AMD_JACOBIAN_ANALYTIC");
    for (int b = 0; b < h->B; ++b)
      if (h->fleet.band_scene[b] >= h->fleet.n_scenes) {
        char buf[160];
        std::snprintf(buf, sizeof buf, "band %d maps to scene %d, but %d scenes are set (teb_amd_set_band_scenes)", b, h->fleet.band_scene[b], h->fleet.n_scenes);
        return fail(TEB_AMD_ERR_INVALID_ARG, buf);
      }
#endif
  }
  OptArgs a;
  std::memset(&a, 0, sizeof a);
  a.inner = inner; a.outer = outer; a.compute_cost = cost_mode; a.no_near_cache = h->opt.no_near_cache != 0; a.band_ldlt = (fleet ? h->fleet.layout : h->layout).solver == SOLVER_BANDG ? 0 : h->band_ldlt; a.Hband = h->Hband.p; a.hband_stride = h->hband_stride;
  a.obst_scale = obst_cost_scale; a.via_scale = viapoint_cost_scale; a.alt_time = alternative_time_cost;
  if (h->iter_log_on) { a.iter_log = h->iter_log.p; a.iter_log_cap = TEB_AMD_ITERATION_LOG_ROWS; }
  if (h->phase_log_on) a.phase_log = h->phase_log.p;
#ifdef TEB_PROFILE
  a.dbg_H = h->dbg_H.p;
#endif
  h->last_inner = inner;
  return launch(h, a);
}
}  // namespace

int teb_amd_optimize_batch(teb_amd_handle_t* h, int32_t inner, int32_t outer, int32_t compute_cost, double obst_cost_scale,
                           double viapoint_cost_scale, int32_t alternative_time_cost) {
  if (int rc = check_handle(h)) return rc;
  return optimize_batch(h, inner, outer, compute_cost != 0 ? 1 : 0, obst_cost_scale, viapoint_cost_scale, alternative_time_cost);
}

int teb_amd_optimize_batch_per_class(teb_amd_handle_t* h, int32_t inner, int32_t outer, int32_t compute_cost_afterwards) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_optimize_batch_per_class"))) return rc;
  return optimize_batch(h, inner, outer, compute_cost_afterwards != 0 ? kCostPerClass : 0, 1.0, 1.0, 0);
}

// g2o's per-iteration console line ("iteration= i chi2= .. lambda= .. levenbergIter= ..", printed when optimization_verbose sets
// SparseOptimizer::setVerbose, src/optimal_planner.cpp:384) as data: one row per LM iteration of the last teb_amd_optimize_batch.
int teb_amd_set_iteration_log(teb_amd_handle_t* h, int32_t enable) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (enable && !h->iter_log.p) {
    const size_t count = (size_t)h->max_tebs * TEB_AMD_ITERATION_LOG_ROWS * 4;
    HIPCHK(h->iter_log.alloc(count));
    HIPCHK(hipMemsetAsync(h->iter_log.p, 0, count * sizeof(double), h->stream));
  }
  h->iter_log_on = enable != 0;
  return TEB_AMD_OK;
}

// Where a launch spends its time, measured on the product kernel itself: shader cycles per phase of every band's workgroup (lane 0,
// s_memtime at the phase boundaries of the outer / LM loop; kPhaseLogSlots values per band, teb_amd_debug.h names them).
static_assert(kPhaseLogSlots == TEB_AMD_PHASE_LOG_SLOTS, "teb_amd_debug.h and teb_device.hpp disagree");
int teb_amd_set_phase_log(teb_amd_handle_t* h, int32_t enable) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (enable && !h->phase_log.p) {
    const size_t count = (size_t)h->max_tebs * kPhaseLogSlots;
    HIPCHK(h->phase_log.alloc(count));
    HIPCHK(hipMemsetAsync(h->phase_log.p, 0, count * sizeof(double), h->stream));
  }
  h->phase_log_on = enable != 0;
  return TEB_AMD_OK;
}
int teb_amd_get_phase_log(teb_amd_handle_t* h, double* cycles, int32_t capacity_bands, int32_t* bands) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!h->phase_log_on || !h->phase_log.p) return fail(TEB_AMD_ERR_INVALID_ARG, "the phase log is off (teb_amd_set_phase_log)");
  if (!cycles || capacity_bands < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  const int nb = std::min((int)capacity_bands, h->B);
  if (nb > 0) HIPCHK(hipMemcpyAsync(cycles, h->phase_log.p, (size_t)nb * kPhaseLogSlots * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (bands) *bands = nb;
  return TEB_AMD_OK;
}

int teb_amd_get_iteration_log(teb_amd_handle_t* h, int32_t b, double* rows, int32_t capacity_rows, int32_t* n_rows) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!h->iter_log_on || !h->iter_log.p) return fail(TEB_AMD_ERR_INVALID_ARG, "the iteration log is off (teb_amd_set_iteration_log)");
  if (b < 0 || b >= h->B || !rows || !n_rows || capacity_rows < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_get_iteration_log: bad arguments");
  int iters = 0;
  HIPCHK(hipMemcpyAsync(&iters, h->bands.iters.p + b, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  int nr = std::min(std::min(iters, (int)TEB_AMD_ITERATION_LOG_ROWS), (int)capacity_rows);
  if (nr < 0) nr = 0;
  if (nr > 0) {
    HIPCHK(hipMemcpyAsync(rows, h->iter_log.p + (size_t)b * TEB_AMD_ITERATION_LOG_ROWS * 4, (size_t)nr * 4 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  *n_rows = nr;
  return TEB_AMD_OK;
}

int teb_amd_synchronize(teb_amd_handle_t* h) {
  int rc = check_handle(h);
  if (rc) return rc;
  return synced(h);
}

int teb_amd_get_results(teb_amd_handle_t* h, teb_amd_results_t* out) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!out) return fail(TEB_AMD_ERR_INVALID_ARG, "null results");
  const int B = h->B;
  if (B == 0) return TEB_AMD_OK;   // an empty handle has no results to copy (a grid of 0 workgroups would be a launch error)
  if (h->pack_host.p && 6 * (size_t)B <= kPackMaxDoubles) {   // six result columns in one gather + one copy
    LAUNCH(pack_results_kernel, dim3((B + 255) / 256), dim3(256), 0, h->stream, h->pack_dev.p, B, h->bands.status.p, h->bands.iters.p, h->bands.trials.p, h->bands.chi2.p, h->bands.cost.p,
           h->bands.lambda.p);
    HIPCHK(hipMemcpyAsync(h->pack_host.p, h->pack_dev.p, 6 * (size_t)B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    const double* m = h->pack_host.p;
    for (int b = 0; b < B; ++b) {
      if (out->status) out->status[b] = (int32_t)m[b];
      if (out->lm_iterations) out->lm_iterations[b] = (int32_t)m[B + b];
      if (out->lm_trials) out->lm_trials[b] = (int32_t)m[2 * B + b];
      if (out->chi2) out->chi2[b] = m[3 * B + b];
      if (out->cost) out->cost[b] = m[4 * B + b];
      if (out->lambda) out->lambda[b] = m[5 * B + b];
    }
    return TEB_AMD_OK;
  }
  if (out->status) HIPCHK(hipMemcpyAsync(out->status, h->bands.status.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (out->lm_iterations) HIPCHK(hipMemcpyAsync(out->lm_iterations, h->bands.iters.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (out->lm_trials) HIPCHK(hipMemcpyAsync(out->lm_trials, h->bands.trials.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (out->chi2) HIPCHK(hipMemcpyAsync(out->chi2, h->bands.chi2.p, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->cost) HIPCHK(hipMemcpyAsync(out->cost, h->bands.cost.p, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (out->lambda) HIPCHK(hipMemcpyAsync(out->lambda, h->bands.lambda.p, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

int teb_amd_select_best(teb_amd_handle_t* h, int32_t last_best, int32_t initial_plan, int32_t* best, double* best_cost) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_select_best"))) return rc;
  if (!best) return fail(TEB_AMD_ERR_INVALID_ARG, "null output");
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs uploaded");
  if (last_best >= h->B) last_best = -1;
  if (initial_plan >= h->B) initial_plan = -1;
  LAUNCH(select_best_kernel, dim3(1), dim3(kThreads), 0, h->stream, h->bands.cost.p, h->B, last_best, initial_plan, h->cfg.selection_cost_hysteresis,
         h->cfg.selection_prefer_initial_plan, h->sel_cost.p, h->sel_idx.p);
  double rec[2];   // one 16-byte copy
  HIPCHK(hipMemcpyAsync(rec, h->sel_cost.p, sizeof(rec), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *best = (int32_t)rec[1];
  if (best_cost) *best_cost = rec[0];
  return TEB_AMD_OK;
}

// ---- multi-GPU: the selection exchange (teb_comm.hpp) --------------------------------------------------------------------------------
#define NCCLCHK(expr)                                                                                                     \
  do {                                                                                                                    \
    int _r = (expr);                                                                                                      \
    if (_r != kRcclSuccess) return fail(TEB_AMD_ERR_HIP, std::string(#expr) + " -> " + rccl().GetErrorString(_r));        \
  } while (0)

int teb_amd_comm_unique_id(char id[TEB_AMD_COMM_ID_BYTES]) {
  static_assert(sizeof(rccl_unique_id_t) == TEB_AMD_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  if (!id) return fail(TEB_AMD_ERR_INVALID_ARG, "null id buffer");
  if (!rccl().load()) return fail(TEB_AMD_ERR_UNSUPPORTED, rccl().error);
  rccl_unique_id_t u;
  NCCLCHK(rccl().GetUniqueId(&u));
  std::memcpy(id, &u, sizeof(u));
  return TEB_AMD_OK;
}

int teb_amd_comm_create(const char id[TEB_AMD_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device, teb_amd_comm_t** out) {
  if (!id || !out || world < 1 || rank < 0 || rank >= world) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_comm_create: bad arguments");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TEB_AMD_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return fail(TEB_AMD_ERR_INVALID_ARG, "device ordinal out of range");
  if (!rccl().load()) return fail(TEB_AMD_ERR_UNSUPPORTED, rccl().error);
  HIPCHK(hipSetDevice(device));
  teb_amd_comm* c = new teb_amd_comm();
  c->rank = rank; c->world = world; c->device = device;
  rccl_unique_id_t u;
  std::memcpy(&u, id, sizeof(u));
  int r = rccl().CommInitRank(&c->comm, world, u, rank);
  if (r != kRcclSuccess) { delete c; return fail(TEB_AMD_ERR_HIP, std::string("ncclCommInitRank -> ") + rccl().GetErrorString(r)); }
  if (hipMalloc(reinterpret_cast<void**>(&c->rec), 2 * sizeof(double)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&c->all), 2 * (size_t)world * sizeof(double)) != hipSuccess) {
    teb_amd_comm_destroy(c);
    return fail(TEB_AMD_ERR_HIP, "teb_amd_comm_create: device allocation failed");
  }
  *out = c;
  return TEB_AMD_OK;
}

void teb_amd_comm_destroy(teb_amd_comm_t* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->comm && rccl().lib) (void)rccl().CommDestroy(c->comm);
  if (c->rec) (void)hipFree(c->rec);
  if (c->all) (void)hipFree(c->all);
  if (c->msg) (void)hipFree(c->msg);
  delete c;
}

// A collective like teb_amd_broadcast_band: whatever is wrong on THIS rank (bad handle, a handle on another device than the communicator's,
// a failed launch) must not keep it out of the all-gather - the peers would wait for ever. Such a rank contributes the
// unusable record (DBL_MAX, -1), which no other rank can pick, and returns its own error AFTER the collective; the peers get the best
// band of the ranks that had one. Only a rank without a communicator cannot take part at all.
int teb_amd_select_best_distributed(teb_amd_handle_t* h, teb_amd_comm_t* c, int32_t global_offset, int32_t last_best_global,
                                    int32_t initial_plan_global, int32_t* best_global, double* best_cost, int32_t* owner_rank) {
  if (!c || !c->comm) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_select_best_distributed: null communicator");
  int local = TEB_AMD_OK;
  std::string why;
  if (check_handle(h)) { local = TEB_AMD_ERR_INVALID_ARG; why = "bad handle"; }
  else if (h->fleet.n_scenes > 0) { local = TEB_AMD_ERR_INVALID_ARG; why = "not available while scenes are set (fleet mode); call teb_amd_clear_scenes first"; }
  else if (!best_global) { local = TEB_AMD_ERR_INVALID_ARG; why = "null output"; }
  else if (c->device != h->device) { local = TEB_AMD_ERR_INVALID_ARG; why = "communicator and handle live on different devices"; }
  (void)hipSetDevice(c->device);
  hipStream_t stream = local == TEB_AMD_OK ? h->stream : nullptr;   // (a rank with an unusable handle takes part on the null stream)
  if (local == TEB_AMD_OK) {
    const int have = h->B > 0;
    if (have) {   // local arg-min with the multipliers applied where this rank owns the favoured candidates
      int lb = last_best_global - global_offset, ip = initial_plan_global - global_offset;
      if (last_best_global < 0 || lb < 0 || lb >= h->B) lb = -1;
      if (initial_plan_global < 0 || ip < 0 || ip >= h->B) ip = -1;
      hipLaunchKernelGGL(select_best_kernel, dim3(1), dim3(kThreads), 0, stream, h->bands.cost.p, h->B, lb, ip,
                         h->cfg.selection_cost_hysteresis, h->cfg.selection_prefer_initial_plan, h->sel_cost.p, h->sel_idx.p);
    }
    hipLaunchKernelGGL(pack_record_kernel, dim3(1), dim3(64), 0, stream, h->sel_cost.p, h->sel_idx.p, global_offset, have, c->rec);
    if (hipGetLastError() != hipSuccess) { local = TEB_AMD_ERR_HIP; why = "local selection kernels failed to launch"; }
  }
  if (local != TEB_AMD_OK) {
    static const double none[2] = {1.7976931348623157e308, -1.0};   // (static: the copy is asynchronous)
    (void)hipMemcpyAsync(c->rec, none, sizeof(none), hipMemcpyHostToDevice, stream);
  }
  NCCLCHK(rccl().AllGather(c->rec, c->all, 2, kRcclFloat64, c->comm, stream));
  std::vector<double> all(2 * (size_t)c->world);
  HIPCHK(hipMemcpyAsync(all.data(), c->all, all.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  double bc; int bi, owner;
  world_argmin(all.data(), c->world, &bi, &bc, &owner);
  // the peers' choice is reported even to the rank that failed (it has to follow them into teb_amd_broadcast_band, a collective too)
  if (best_global) *best_global = bi;
  if (best_cost) *best_cost = bc;
  if (owner_rank) *owner_rank = owner;
  if (local != TEB_AMD_OK) return fail(local, "teb_amd_select_best_distributed: " + why + " (this rank sent an unusable record; its peers were not held up)");
  return TEB_AMD_OK;
}

// A collective: no rank may leave before the peers are released. Everything that can go wrong on ONE rank (an index out of range on the
// owner, an allocation failure, capacities that differ between the ranks) is therefore found out by all ranks together - an all-gather of
// (status, capacity) per rank - BEFORE the broadcast, and every rank returns the same verdict. Only a rank without a communicator cannot
// take part at all (TEB_AMD_ERR_INVALID_ARG there; its peers then wait in the all-gather like in any collective a rank never enters).
int teb_amd_broadcast_band(teb_amd_handle_t* h, teb_amd_comm_t* c, int32_t owner_rank, int32_t local_index, int32_t capacity, int32_t* n,
                           double* x, double* y, double* theta, double* dt) {
  if (!c || !c->comm) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_broadcast_band: null communicator");
  int local = TEB_AMD_OK;
  std::string why;
  if (check_handle(h)) { local = TEB_AMD_ERR_INVALID_ARG; why = "bad handle"; }
  else if (h->fleet.n_scenes > 0) { local = TEB_AMD_ERR_INVALID_ARG; why = "not available while scenes are set (fleet mode); call teb_amd_clear_scenes first"; }
  else if (!n || !x || !y || !theta || !dt || capacity < 2) { local = TEB_AMD_ERR_INVALID_ARG; why = "null output / capacity < 2"; }
  else if (owner_rank < 0 || owner_rank >= c->world) { local = TEB_AMD_ERR_INVALID_ARG; why = "owner_rank out of range"; }
  else if (c->rank == owner_rank && (local_index < 0 || local_index >= h->B)) { local = TEB_AMD_ERR_INVALID_ARG; why = "local_index out of range on the owner"; }
  (void)hipSetDevice(c->device);
  hipStream_t stream = h ? h->stream : nullptr;   // (a rank with a bad handle still takes part, on the null stream)
  const size_t count = capacity >= 2 ? 3 + 4 * (size_t)capacity : 0;   // n, four strips, the band's statistics
  if (local == TEB_AMD_OK && c->msg_cap < count) {
    if (c->msg) (void)hipFree(c->msg);
    c->msg = nullptr; c->msg_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&c->msg), count * sizeof(double)) != hipSuccess) { local = TEB_AMD_ERR_HIP; why = "message buffer allocation failed"; }
    else c->msg_cap = count;
  }
  // round 1: (status, capacity) of every rank
  const double mine[2] = {(double)local, (double)capacity};
  std::vector<double> all(2 * (size_t)c->world);
  if (hipMemcpyAsync(c->rec, mine, sizeof(mine), hipMemcpyHostToDevice, stream) != hipSuccess) return fail(TEB_AMD_ERR_HIP, "teb_amd_broadcast_band: staging copy failed");
  NCCLCHK(rccl().AllGather(c->rec, c->all, 2, kRcclFloat64, c->comm, stream));
  HIPCHK(hipMemcpyAsync(all.data(), c->all, all.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  for (int r = 0; r < c->world; ++r) {
    if ((int)all[2 * r] != TEB_AMD_OK)
      return fail(r == c->rank ? local : TEB_AMD_ERR_INVALID_ARG,
                  r == c->rank ? "teb_amd_broadcast_band: " + why : "teb_amd_broadcast_band: rank " + std::to_string(r) + " reported an error; no band was sent");
    if ((int)all[2 * r + 1] != capacity)
      return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_broadcast_band: `capacity` differs between the ranks (rank " + std::to_string(r) + " passed " +
                                               std::to_string((int)all[2 * r + 1]) + ", this rank " + std::to_string(capacity) + ")");
  }
  // round 2: the strip itself
  if (c->rank == owner_rank)
    hipLaunchKernelGGL(pack_band_kernel, dim3((capacity + 255) / 256), dim3(256), 0, stream, h->bands.strips.n.p, h->bands.strips.x.p, h->bands.strips.y.p, h->bands.strips.th.p, h->bands.strips.dt.p,
                       local_index, h->stride, capacity, c->msg, h->bands.chi2.p, h->bands.iters.p, h->bands.last_iters.p, h->cfg.divergence_detection_enable != 0,
                       h->last_inner);
  const bool packed = hipGetLastError() == hipSuccess;   // (a failed pack still enters the broadcast; what arrives is then rejected below)
  NCCLCHK(rccl().Broadcast(c->msg, c->msg, count, kRcclFloat64, owner_rank, c->comm, stream));
  std::vector<double> host(count);
  HIPCHK(hipMemcpyAsync(host.data(), c->msg, count * sizeof(double), hipMemcpyDeviceToHost, stream));
  HIPCHK(hipStreamSynchronize(stream));
  if (!packed) return fail(TEB_AMD_ERR_HIP, "teb_amd_broadcast_band: packing the band failed on the owner");
  const int nb = (int)host[0];
  *n = nb;
  if (nb > capacity) return fail(TEB_AMD_ERR_CAPACITY, "the winner has more poses than `capacity`");
  std::memcpy(x, host.data() + 1, capacity * sizeof(double));
  std::memcpy(y, host.data() + 1 + capacity, capacity * sizeof(double));
  std::memcpy(theta, host.data() + 1 + 2 * (size_t)capacity, capacity * sizeof(double));
  std::memcpy(dt, host.data() + 1 + 3 * (size_t)capacity, capacity * sizeof(double));
  c->band_stats_available = host[1 + 4 * (size_t)capacity] != 0.0;
  c->band_stats_back_chi2 = host[2 + 4 * (size_t)capacity];
  return TEB_AMD_OK;
}

int teb_amd_comm_last_band_statistics(const teb_amd_comm_t* c, int32_t* available, double* back_chi2) {
  if (!c || !available || !back_chi2) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_comm_last_band_statistics: null argument");
  *available = c->band_stats_available; *back_chi2 = c->band_stats_back_chi2;
  return TEB_AMD_OK;
}

int teb_amd_debug_world_argmin(const double* records, int32_t world, int32_t* best_global, double* best_cost, int32_t* owner_rank) {
  if (!records || world < 1 || !best_global) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_debug_world_argmin: bad arguments");
  int bi, owner; double bc;
  world_argmin(records, world, &bi, &bc, &owner);
  *best_global = bi;
  if (best_cost) *best_cost = bc;
  if (owner_rank) *owner_rank = owner;
  return TEB_AMD_OK;
}

// ---- f1 / f2: producers and consumers of the device-resident strips (kernels in teb_strip.hpp) ---------------------------------
namespace {

// slots >= B join the batch as BandAttrs::fresh()
int extend_batch(teb_amd_handle* h, int b) {
  if (b < 0 || b >= h->max_tebs) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB slot out of range");
  for (int k = h->B; k <= b; ++k) {
    const BandAttrs a = BandAttrs::fresh();
    const int two = 2;
    HIPCHK(hipMemcpyAsync(h->bands.has_vs.p + k, &a.has_vs, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->bands.has_vg.p + k, &a.has_vg, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->bands.rotdir.p + k, &a.rotdir, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->bands.via_en.p + k, &a.via_en, sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->bands.optimized.p + k, 0, sizeof(int), h->stream));   // a new TebOptimalPlanner: optimized_(false)
    HIPCHK(hipMemcpyAsync(h->bands.vs.p + 3 * k, a.vs, sizeof(a.vs), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->bands.vg.p + 3 * k, a.vg, sizeof(a.vg), hipMemcpyHostToDevice, h->stream));
    if (k < b) {   // a skipped slot becomes the trivial two-pose band at the origin so that the batch stays well-formed
      const double zz[2] = {0, 0}, dd[2] = {0.1, 0};
      const size_t o = (size_t)k * h->stride;
      HIPCHK(hipMemcpyAsync(h->bands.strips.x.p + o, zz, sizeof(zz), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(h->bands.strips.y.p + o, zz, sizeof(zz), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(h->bands.strips.th.p + o, zz, sizeof(zz), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(h->bands.strips.dt.p + o, dd, sizeof(dd), hipMemcpyHostToDevice, h->stream));
      HIPCHK(hipMemcpyAsync(h->bands.strips.n.p + k, &two, sizeof(int), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));   // the small host temporaries above
  }
  if (b >= h->B) h->B = b + 1;
  return TEB_AMD_OK;
}

int finish_init(teb_amd_handle* h) {
  HIPCHK(hipGetLastError());
  int err = 0;
  HIPCHK(hipMemcpyAsync(&err, h->err_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  h->bands_changed();
  if (err) return fail(TEB_AMD_ERR_CAPACITY, "initTrajectoryToGoal: the band needs more poses than max_poses");
  return TEB_AMD_OK;
}

int stage(teb_amd_handle* h, int n, const double* px, const double* py, const double* pyaw) {
  if (n < 1 || !px || !py) return fail(TEB_AMD_ERR_INVALID_ARG, "empty plan / path");
  if (n > h->stride + 1) return fail(TEB_AMD_ERR_CAPACITY, "plan / path longer than max_poses + 1");
  HIPCHK(hipMemcpyAsync(h->stage_x.p, px, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->stage_y.p, py, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (pyaw) HIPCHK(hipMemcpyAsync(h->stage_yaw.p, pyaw, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(h->err_flag.p, 0, sizeof(int), h->stream));
  return TEB_AMD_OK;
}

int run_consumers(teb_amd_handle* h, int look_ahead, int prevent) {
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs on the device");
  if (h->consumers_valid && h->consumers_la == look_ahead && h->consumers_prevent == prevent) return TEB_AMD_OK;
  if (h->fleet.n_scenes > 0 && !h->fleet.classes.empty()) {   // a class map: every band under the configuration of its scene's class
    if (int rc = check_band_scenes(h, h->B)) return rc;
    LAUNCH(consumers_fleet_kernel, dim3(h->B), dim3(kThreads), 0, h->stream, h->fleet.cfgs.p, h->fleet.class_of_scene.p, h->fleet.scene_of.p, batch_of(h), look_ahead, prevent,
           h->out_cmd.p, h->out_prof.p, h->out_traj.p);
  } else
    LAUNCH(consumers_kernel, dim3(h->B), dim3(kThreads), 0, h->stream, h->cfg, batch_of(h), look_ahead, prevent, h->out_cmd.p, h->out_prof.p, h->out_traj.p);
  h->consumers_valid = true; h->consumers_la = look_ahead; h->consumers_prevent = prevent;
  return TEB_AMD_OK;
}

int band_n(teb_amd_handle* h, int b, int* n) {
  if (b < 0 || b >= h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  HIPCHK(hipMemcpyAsync(n, h->bands.strips.n.p + b, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

}  // namespace

int teb_amd_init_trajectory_line(teb_amd_handle_t* h, int32_t b, const double* start, const double* goal, double diststep,
                                 double max_vel_x, int32_t min_samples, int32_t guess_backwards_motion) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!start || !goal) return fail(TEB_AMD_ERR_INVALID_ARG, "null start / goal");
  if ((rc = extend_batch(h, b))) return rc;
  HIPCHK(hipMemsetAsync(h->err_flag.p, 0, sizeof(int), h->stream));
  hipLaunchKernelGGL(init_line_kernel, dim3(1), dim3(kThreads), 0, h->stream, batch_of(h), b, start[0], start[1], start[2], goal[0],
                     goal[1], goal[2], diststep, max_vel_x, min_samples, guess_backwards_motion, h->err_flag.p);
  return finish_init(h);
}

int teb_amd_init_trajectory_plan(teb_amd_handle_t* h, int32_t b, int32_t n_plan, const double* plan_x, const double* plan_y,
                                 const double* plan_yaw, double max_vel_x, double max_vel_theta, int32_t estimate_orient,
                                 int32_t min_samples, int32_t guess_backwards_motion) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!plan_yaw) return fail(TEB_AMD_ERR_INVALID_ARG, "null plan_yaw");
  if ((rc = extend_batch(h, b))) return rc;
  if ((rc = stage(h, n_plan, plan_x, plan_y, plan_yaw))) return rc;
  hipLaunchKernelGGL(init_plan_kernel, dim3(1), dim3(kThreads), 0, h->stream, batch_of(h), b, n_plan, h->stage_x.p, h->stage_y.p,
                     h->stage_yaw.p, max_vel_x, max_vel_theta, estimate_orient, min_samples, guess_backwards_motion, h->err_flag.p);
  return finish_init(h);
}

int teb_amd_init_trajectory_path(teb_amd_handle_t* h, int32_t b, int32_t n_path, const double* path_x, const double* path_y,
                                 double max_vel_x, double max_vel_theta, const double* max_acc_x, const double* start_orientation,
                                 const double* goal_orientation, int32_t min_samples, int32_t guess_backwards_motion) {
  (void)max_vel_theta;   // unused by the reference too (its angular time step code is commented out, timed_elastic_band.hpp:118-140)
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = extend_batch(h, b))) return rc;
  if ((rc = stage(h, n_path, path_x, path_y, nullptr))) return rc;
  hipLaunchKernelGGL(init_path_kernel, dim3(1), dim3(kThreads), 0, h->stream, batch_of(h), b, n_path, h->stage_x.p, h->stage_y.p,
                     max_vel_x, max_acc_x ? 1 : 0, max_acc_x ? *max_acc_x : 0.0, start_orientation ? 1 : 0,
                     start_orientation ? *start_orientation : 0.0, goal_orientation ? 1 : 0, goal_orientation ? *goal_orientation : 0.0,
                     min_samples, guess_backwards_motion, h->err_flag.p);
  return finish_init(h);
}

int teb_amd_update_and_prune(teb_amd_handle_t* h, int32_t b, const double* new_start, const double* new_goal, int32_t min_samples) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs on the device");
  if (b >= h->B || b < -1) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  const double z[3] = {0, 0, 0};
  const double* s = new_start ? new_start : z;
  const double* g = new_goal ? new_goal : z;
  LAUNCH(prune_kernel, dim3(b < 0 ? h->B : 1), dim3(kThreads), 4 * (size_t)h->stride * sizeof(double), h->stream, batch_of(h), b < 0 ? 0 : b, new_start ? 1 : 0,
         s[0], s[1], s[2], new_goal ? 1 : 0, g[0], g[1], g[2], min_samples);
  h->bands_changed();
  return TEB_AMD_OK;
}

namespace {
int set_velocity(teb_amd_handle* h, DevBuf<int>& flag, DevBuf<double>& vel, int b, int fixed, const double* v) {
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs on the device");
  if (b >= h->B || b < -1) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  const int b0 = b < 0 ? 0 : b, b1 = b < 0 ? h->B : b + 1;
  std::vector<int> f(b1 - b0, fixed ? 1 : 0);
  HIPCHK(hipMemcpyAsync(flag.p + b0, f.data(), f.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  std::vector<double> vv;
  if (v) {
    for (int k = b0; k < b1; ++k) { vv.push_back(v[0]); vv.push_back(v[1]); vv.push_back(v[2]); }
    HIPCHK(hipMemcpyAsync(vel.p + 3 * b0, vv.data(), vv.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  h->bands_changed(-1, false);
  return TEB_AMD_OK;
}
}  // namespace

int teb_amd_set_velocity_start(teb_amd_handle_t* h, int32_t b, int32_t fixed, const double* v) {
  int rc = check_handle(h);
  if (rc) return rc;
  return set_velocity(h, h->bands.has_vs, h->bands.vs, b, fixed, v);
}

int teb_amd_set_velocity_goal(teb_amd_handle_t* h, int32_t b, int32_t fixed, const double* v) {
  int rc = check_handle(h);
  if (rc) return rc;
  return set_velocity(h, h->bands.has_vg, h->bands.vg, b, fixed, v);
}

int teb_amd_get_pose_counts(teb_amd_handle_t* h, int32_t* n, int32_t* count) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (count) *count = h->B;
  if (n && h->B > 0) {
    HIPCHK(hipMemcpyAsync(n, h->bands.strips.n.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  return TEB_AMD_OK;
}

int teb_amd_get_velocity_command(teb_amd_handle_t* h, int32_t b, int32_t look_ahead_poses, int32_t prevent_look_ahead_poses_near_goal,
                                 double* vx, double* vy, double* omega, int32_t* ok) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (b < 0 || b >= h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  if ((rc = run_consumers(h, look_ahead_poses, prevent_look_ahead_poses_near_goal))) return rc;
  double c[4];
  HIPCHK(hipMemcpyAsync(c, h->out_cmd.p + 4 * (size_t)b, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (vx) *vx = c[0]; if (vy) *vy = c[1]; if (omega) *omega = c[2]; if (ok) *ok = c[3] != 0;
  return TEB_AMD_OK;
}

int teb_amd_get_velocity_profile(teb_amd_handle_t* h, int32_t b, double* out, int32_t capacity_rows, int32_t* rows) {
  int rc = check_handle(h);
  if (rc) return rc;
  int n = 0;
  if ((rc = band_n(h, b, &n))) return rc;
  if (rows) *rows = n + 1;
  if (!out) return TEB_AMD_OK;
  if (capacity_rows < n + 1) return fail(TEB_AMD_ERR_CAPACITY, "velocity profile needs n+1 rows");
  if ((rc = run_consumers(h, h->consumers_valid ? h->consumers_la : 1, h->consumers_valid ? h->consumers_prevent : 0))) return rc;
  HIPCHK(hipMemcpyAsync(out, h->out_prof.p + (size_t)b * (h->stride + 1) * 3, (size_t)(n + 1) * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

int teb_amd_get_full_trajectory(teb_amd_handle_t* h, int32_t b, double* out, int32_t capacity_rows, int32_t* rows) {
  int rc = check_handle(h);
  if (rc) return rc;
  int n = 0;
  if ((rc = band_n(h, b, &n))) return rc;
  if (rows) *rows = n;
  if (!out) return TEB_AMD_OK;
  if (capacity_rows < n) return fail(TEB_AMD_ERR_CAPACITY, "trajectory needs n rows");
  if ((rc = run_consumers(h, h->consumers_valid ? h->consumers_la : 1, h->consumers_valid ? h->consumers_prevent : 0))) return rc;
  HIPCHK(hipMemcpyAsync(out, h->out_traj.p + (size_t)b * h->stride * 7, (size_t)n * 7 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

// TebOptimalPlanner::hasDiverged (src/optimal_planner.cpp:1023-1039) reads optimizer_->batchStatistics().back().chi2. g2o sizes that
// vector to the REQUESTED iteration count of the last optimize() call and fills one entry per executed iteration: when the LM loop of
// that call terminated early the last entry is still zero-initialised and the planner does not report a divergence whatever chi2 was
// reached. The kernel returns the number of iterations of the band's last optimize() call beside the chi2 after its last iteration.
static bool diverged_rule(const teb_amd_config_t& c, int last_inner, int iters, int last_iters, double chi2) {
  if (!c.divergence_detection_enable) return false;                          // :1026-1027
  if (iters <= 0 || last_inner <= 0) return false;                           // no statistics yet, :1031-1033
  const double back = last_iters == last_inner ? chi2 : 0.0;                 // .back() of a vector resized to `iterations`
  return back > c.divergence_detection_max_chi_squared;                      // :1038
}

int teb_amd_has_diverged(teb_amd_handle_t* h, int32_t b, int32_t* diverged) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (b < 0 || b >= h->B || !diverged) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  *diverged = 0;
  const teb_amd_config_t& c = band_cfg(h, b);   // of the band's class in fleet mode
  if (!c.divergence_detection_enable) return TEB_AMD_OK;
  double chi2 = 0; int iters = 0, last = 0;
  HIPCHK(hipMemcpyAsync(&chi2, h->bands.chi2.p + b, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&iters, h->bands.iters.p + b, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(&last, h->bands.last_iters.p + b, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  *diverged = diverged_rule(c, h->last_inner, iters, last, chi2);
  return TEB_AMD_OK;
}

// What optimizer_->batchStatistics() of every resident band would hold after the last teb_amd_optimize_batch: available [count] =
// the vector is not empty (statistics were switched on for that call, src/optimal_planner.cpp:331, and optimize() ran), back_chi2
// [count] = .back().chi2 (zero when the band's last optimize() call stopped before its last requested iteration). A binding keeps
// the pair per planner object and applies hasDiverged's rule to the configuration it holds at that time.
int teb_amd_get_batch_statistics(teb_amd_handle_t* h, int32_t* available, double* back_chi2) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!available || !back_chi2) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  const int B = h->B;
  if (B <= 0) return TEB_AMD_OK;
  std::vector<double> chi2(B); std::vector<int> iters(B), last(B);
  HIPCHK(hipMemcpyAsync(chi2.data(), h->bands.chi2.p, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(iters.data(), h->bands.iters.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(last.data(), h->bands.last_iters.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  for (int b = 0; b < B; ++b) {
    available[b] = band_cfg(h, b).divergence_detection_enable && iters[b] > 0 && h->last_inner > 0;
    back_chi2[b] = (available[b] && last[b] == h->last_inner) ? chi2[b] : 0.0;
  }
  return TEB_AMD_OK;
}

// ---- f4: feasibility of the resident bands against a costmap grid (kernel in teb_feasibility.hpp) --------------------------------------
int teb_amd_set_costmap(teb_amd_handle_t* h, const uint8_t* cells, int32_t size_x, int32_t size_y, double resolution, double origin_x,
                        double origin_y) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!cells || size_x <= 0 || size_y <= 0 || !(resolution > 0)) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_costmap: bad grid");
  const size_t bytes = (size_t)size_x * size_y;
  h->cm = GridDev{};   // (it holds the address of the cells, which may move now: a HIP error from here on leaves no costmap)
  HIPCHK(ensure(h->cm_cells, bytes));
  HIPCHK(hipMemcpyAsync(h->cm_cells.p, cells, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // the caller's buffer may go away
  h->cm = GridDev{h->cm_cells.p, size_x, size_y, resolution, origin_x, origin_y};
  return TEB_AMD_OK;
}

namespace {
// What the two feasibility calls share. Their argument checks: `given` says that the call's pointers and footprint size are usable.
int check_feasibility_arguments(bool given, const char* what, double inscribed_radius, double min_res_angular) {
  if (!given) return fail(TEB_AMD_ERR_INVALID_ARG, what);
  if (!(inscribed_radius > 0) || !(min_res_angular > 0)) return fail(TEB_AMD_ERR_INVALID_ARG, "inscribed_radius and the angular resolution must be > 0");
  return TEB_AMD_OK;
}
// ... and `count` checks in one launch: the footprint upload (nf entries per plane: one footprint, or those of all specs of
// teb_amd_is_trajectory_feasible_per_class one after the other), the output block [feasible | first_infeasible] count each + the overflow
// word with its one download, and the refusal of more than 2^22 samples. launch(fp_x, fp_y, feasible, first_infeasible, overflow) runs
// the call's kernel on the device arrays.
extern "C++" template <class Launch>
int run_feasibility(teb_amd_handle* h, int count, int nf, const double* fx, const double* fy, int32_t* feasible, int32_t* first_infeasible, Launch launch) {
  if (h->stride > 1024) return fail(TEB_AMD_ERR_CAPACITY, "feasibility check supports bands up to 1024 poses");
  const size_t plane = std::max<size_t>((size_t)kMaxFeasFootprint, (size_t)nf);
  HIPCHK(ensure(h->cm_fp, 2 * plane));
  HIPCHK(ensure(h->cm_out, 2 * (size_t)h->max_tebs + 1));
  int* ovf = h->cm_out.p + 2 * (size_t)count;
  HIPCHK(hipMemcpyAsync(h->cm_fp.p, fx, nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->cm_fp.p + plane, fy, nf * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemsetAsync(ovf, 0, sizeof(int), h->stream));
  if (int rc = launch(h->cm_fp.p, h->cm_fp.p + plane, h->cm_out.p, h->cm_out.p + count, ovf)) return rc;
  std::vector<int> out(2 * (size_t)count + 1);
  HIPCHK(hipMemcpyAsync(out.data(), h->cm_out.p, out.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // (the caller's footprint, and what launch() uploaded, are read until here)
  if (out[2 * (size_t)count]) return fail(TEB_AMD_ERR_CAPACITY, "feasibility check: more than 2^22 interpolated samples requested (inscribed radius / angular resolution too small)");
  for (int k = 0; k < count; ++k) { feasible[k] = out[k]; if (first_infeasible) first_infeasible[k] = out[count + k]; }
  return TEB_AMD_OK;
}
}  // namespace

int teb_amd_is_trajectory_feasible(teb_amd_handle_t* h, int32_t b, int32_t nf, const double* fx, const double* fy, double inscribed_radius,
                                   double min_res_angular, int32_t look_ahead_idx, double lookahead_distance, int32_t* feasible,
                                   int32_t* first_infeasible) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (h->cm.sx <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_is_trajectory_feasible: no costmap (teb_amd_set_costmap)");
  if ((rc = check_feasibility_arguments(feasible && nf >= 1 && nf <= kMaxFeasFootprint && fx && fy, "bad footprint / output", inscribed_radius, min_res_angular))) return rc;
  if (h->B <= 0 || b >= h->B || b < -1) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  const int first = b < 0 ? 0 : b, count = b < 0 ? h->B : 1;
  return run_feasibility(h, count, nf, fx, fy, feasible, first_infeasible, [&](double* px, double* py, int* fe, int* fi, int* ovf) {
    LAUNCH(feasibility_kernel, dim3(count), dim3(kFeasThreads), 0, h->stream, h->bands.strips.n.p, h->bands.strips.x.p, h->bands.strips.y.p, h->bands.strips.th.p, h->stride, first, h->cm, nf, px, py,
           inscribed_radius, min_res_angular, look_ahead_idx, lookahead_distance, 1 << 22, fe, fi, ovf);
    return (int)TEB_AMD_OK;
  });
}

namespace {
// The H-signatures of the `count` bands of bt (the batch, or the candidate strips of an exploration) into out. fl NULL: against the
// single scene's table, band k at out + k * W, W = M (3-D) or 2 (2-D). Else band k against the table of scene fl->scene_of[k], at
// fl->off[k] (3-D; the offsets uploaded by the caller) or at 2 k (2-D). n_values: values in all.
int launch_signatures(teb_amd_handle* h, const FleetHsigDev* fl, const BatchDev& bt, int count, size_t n_values, double prescaler, double* out) {
  auto& F = h->fleet;
  if (count <= 0) return TEB_AMD_OK;
  int widest = h->M;   // most rows of a table
  if (fl) { widest = 0; for (const HostObst& t : F.tabs) widest = std::max(widest, (int)t.rows()); }
  const size_t strip = (size_t)h->stride * sizeof(double);
  if (agreed_cfg(h, fl != nullptr).include_dynamic_obstacles) {
    if (n_values == 0) return TEB_AMD_OK;
    const bool wide = hsig3d_wide(h->opt.hsig3d_kernel, (long long)n_values);
    const dim3 grid((widest + (wide ? kThreads : kHsTile) - 1) / (wide ? kThreads : kHsTile), count);
    if (!fl && wide) LAUNCH(hsig3d_kernel, grid, dim3(kThreads), 3 * strip, h->stream, scene_of(h), bt, out);
    else if (!fl) LAUNCH(hsig3d_small_kernel, grid, dim3(kThreads), 3 * strip, h->stream, scene_of(h), bt, out);
    else if (wide) LAUNCH(hsig3d_fleet_kernel, grid, dim3(kThreads), 3 * strip, h->stream, *fl, bt, out);
    else LAUNCH(hsig3d_small_fleet_kernel, grid, dim3(kThreads), 3 * strip, h->stream, *fl, bt, out);
    return TEB_AMD_OK;
  }
  bool& products_valid = fl ? F.hs_prod_valid : h->hs_prod_valid;
  if (widest > 0 && !products_valid) {   // the band-independent factor of A_l: once per obstacle table, every scene over its own rows (O(M^2))
    const unsigned blocks = (widest + kThreads - 1) / kThreads;
    if (!fl) LAUNCH(hsig2d_prod_kernel, dim3(blocks), dim3(kThreads), 0, h->stream, scene_of(h), h->hs_pre.p, h->hs_pim.p, h->hs_pex.p);
    else LAUNCH(hsig2d_prod_fleet_kernel, dim3(blocks, F.n_scenes), dim3(kThreads), 0, h->stream, F.scenes.p, F.store.cx.p, F.hs_pre.p, F.hs_pim.p, F.hs_pex.p);
    products_valid = true;
  }
  if (!fl) LAUNCH(hsig2d_kernel, dim3(count), dim3(kThreads), 2 * strip, h->stream, scene_of(h), bt, prescaler, h->hs_pre.p, h->hs_pim.p, h->hs_pex.p, out);
  else LAUNCH(hsig2d_fleet_kernel, dim3(count), dim3(kThreads), 2 * strip, h->stream, *fl, bt, prescaler, F.store.cx.p, F.hs_pre.p, F.hs_pim.p, F.hs_pex.p, out);
  return TEB_AMD_OK;
}

// The signatures of the B resident bands into S at the offsets `off`: one launch into h->hsig [max_tebs * max(max_obstacles, 2)], one
// download. by_scene: against the tables of the scene set (the offsets go to the device for the 3-D kernels), else the single scene's.
int compute_signatures(teb_amd_handle* h, SignatureSet& S, bool by_scene, std::vector<int> off, double prescaler) {
  auto& F = h->fleet;
  const int mode = agreed_cfg(h, by_scene).include_dynamic_obstacles ? 3 : 2;   // homotopy_class_planner.hpp:50
  double* host = S.reserve(std::move(off));
  const size_t total = (size_t)S.off.back();
  FleetHsigDev fl;
  fl.scenes = F.scenes.p; fl.scene_of = F.scene_of.p; fl.off = F.hs_off.p;
  if (by_scene && mode == 3 && total > 0) HIPCHK(hipMemcpyAsync(F.hs_off.p, S.off.data(), S.off.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (int rc = launch_signatures(h, by_scene ? &fl : nullptr, batch_of(h), h->B, total, prescaler, h->hsig.p)) return rc;
  if (total > 0) HIPCHK(hipMemcpyAsync(host, h->hsig.p, total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  S.stamp(mode, prescaler);
  return TEB_AMD_OK;
}
}  // namespace

// ---- f3 (arithmetic core): equivalence classes of the device-resident bands (kernels in teb_hsig.hpp), for the single scene and per
// scene of a fleet batch (the fleet forms of the kernels). Each step is one function over a SignatureSet and BandGroups. ------------------
int teb_amd_compute_h_signatures(teb_amd_handle_t* h, double prescaler, double* values, int32_t* width) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_compute_h_signatures"))) return rc;
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs on the device");
  const int W = h->cfg.include_dynamic_obstacles ? h->M : 2;
  if (width) *width = W;
  if ((rc = compute_signatures(h, h->sigs, false, SignatureSet::fixed_width(h->B, W), prescaler))) return rc;
  if (values) std::copy(h->sigs.values.begin(), h->sigs.values.begin() + h->sigs.off.back(), values);
  return TEB_AMD_OK;
}

int teb_amd_filter_equivalence_classes(teb_amd_handle_t* h, double threshold, int32_t best, int32_t max_number_plans_in_current_class,
                                       int32_t* keep, int32_t* valid, int32_t* reasonable) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_filter_equivalence_classes"))) return rc;
  if (h->sigs.mode == 0 || h->sigs.B != h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "call teb_amd_compute_h_signatures first");
  filter_class_lists(h->sigs, BandGroups(1, h->B, nullptr), threshold, max_number_plans_in_current_class, &best, &h->memory, keep, valid, reasonable);
  return TEB_AMD_OK;
}

int teb_amd_compute_h_signatures_per_scene(teb_amd_handle_t* h, double prescaler, double* values, int64_t capacity_values, int32_t* offset,
                                           int64_t* n_values) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_values) *n_values = 0;
  if ((rc = require_fleet_mode(h, "teb_amd_compute_h_signatures_per_scene"))) return rc;
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs on the device");
  auto& F = h->fleet;
  const int B = h->B;
  if ((rc = check_band_scenes(h, B))) return rc;
  std::vector<int> off(B + 1, 0);
  for (int b = 0; b < B; ++b) off[b + 1] = off[b] + (agreed_cfg(h, true).include_dynamic_obstacles ? (int)F.tabs[F.band_scene[b]].rows() : 2);
  const int64_t total = off[B];
  if (n_values) *n_values = total;
  if (offset) std::copy(off.begin(), off.end(), offset);
  if ((rc = compute_signatures(h, F.sigs, true, std::move(off), prescaler))) return rc;
  if (!values) return TEB_AMD_OK;   // compute only: the signatures stay in the handle for the filter call
  if (capacity_values < total) return fail(TEB_AMD_ERR_CAPACITY, "teb_amd_compute_h_signatures_per_scene: capacity_values is smaller than *n_values (the signatures are kept for the filter call)");
  std::copy(F.sigs.values.begin(), F.sigs.values.begin() + total, values);
  return TEB_AMD_OK;
}

int teb_amd_filter_equivalence_classes_per_scene(teb_amd_handle_t* h, double threshold, const int32_t* best,
                                                 int32_t max_number_plans_in_current_class, int32_t* keep, int32_t* valid, int32_t* reasonable) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_filter_equivalence_classes_per_scene"))) return rc;
  auto& F = h->fleet;
  if (F.sigs.mode == 0 || F.sigs.B != h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "call teb_amd_compute_h_signatures_per_scene first");
  BandGroups G;
  if ((rc = scene_groups(h, h->B, G)) || (rc = check_best_per_scene(G, best, "teb_amd_filter_equivalence_classes_per_scene"))) return rc;
  filter_class_lists(F.sigs, G, threshold, max_number_plans_in_current_class, best, F.memory.data(), keep, valid, reasonable);
  return TEB_AMD_OK;
}

// ---- both ends of a fleet tick per scene (teb_amd.h): a costmap set, the obstacle tables of every scene from its grid, feasibility of one
// band per scene against its own grid, updateAllTEBs of every robot in one launch, the commands of many bands in one call -------------
int teb_amd_set_costmaps(teb_amd_handle_t* h, int32_t n, const uint8_t* cells, const int32_t* size_x, const int32_t* size_y, const double* resolution,
                         const double* origin_x, const double* origin_y) {
  int rc = check_handle(h);
  if (rc) return rc;
  auto& S = h->cms;
  if (n < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_costmaps: negative number of grids");
  if (n == 0) { S.n = 0; S.grids_host.clear(); return TEB_AMD_OK; }
  if (!cells || !size_x || !size_y || !resolution || !origin_x || !origin_y) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_costmaps: null argument");
  if (n > h->max_tebs) return fail(TEB_AMD_ERR_CAPACITY, "more grids than max_tebs");
  // everything is checked before the first upload: on a bad argument the previous set stays
  std::vector<GridDev> g(n);
  std::vector<size_t> first(n);
  size_t bytes = 0;
  for (int s = 0; s < n; ++s) {
    if (size_x[s] <= 0 || size_y[s] <= 0 || !(resolution[s] > 0)) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_set_costmaps: bad grid");
    first[s] = bytes;
    bytes += (size_t)size_x[s] * (size_t)size_y[s];
  }
  if (S.cells.n < bytes) {   // the new buffer before the old one goes: a failed allocation leaves the previous set
    DevBuf<unsigned char> nb;
    if (nb.alloc(bytes) != hipSuccess) { (void)hipGetLastError(); return fail(TEB_AMD_ERR_HIP, "teb_amd_set_costmaps: device allocation failed"); }
    HIPCHK(hipStreamSynchronize(h->stream));
    S.cells = std::move(nb);
  }
  if (!S.grids.p) HIPCHK(S.grids.alloc((size_t)h->max_tebs));
  for (int s = 0; s < n; ++s) g[s] = GridDev{S.cells.p + first[s], size_x[s], size_y[s], resolution[s], origin_x[s], origin_y[s]};
  S.n = 0;   // from here on the previous grids are overwritten: a HIP error leaves no set
  S.grids_host.clear();
  HIPCHK(hipMemcpyAsync(S.cells.p, cells, bytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(S.grids.p, g.data(), (size_t)n * sizeof(GridDev), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // the caller's buffer may go away
  S.grids_host = std::move(g);
  S.n = n;
  return TEB_AMD_OK;
}

// ---- a costmap becomes an obstacle table: updateObstacleContainerWithCostmap (src/teb_local_planner_ros.cpp:478-504, kernels in
// teb_costmap_obstacles.hpp) and the converter slot updateObstacleContainerWithCostmapConverter (:506-549, kernels in
// teb_costmap_polygons.hpp), for the single scene and for a scene set. ONE procedure (convert_costmaps) over a row kind and a route;
// its host rules are teb_costmap_host.hpp --------------------------------------------------------------------------------------------
namespace {
// The write pass of the polygon route and its read-back, the same on both routes but for the launch: the converted rows of the set at
// their prefix offsets of one scratch - first-vertex offsets (from the scene's first vertex on) and vertex coordinates (world), in
// table order - read back once.
extern "C++" template <class Launch>
int write_polygon_rows(teb_amd_handle* h, PolygonRows& K, Launch&& launch) {
  auto& S = h->cmx;
  const size_t rows = (size_t)K.rows, verts = (size_t)K.verts;
  if (rows == 0) return TEB_AMD_OK;
  HIPCHK(ensure(S.poff, rows));
  HIPCHK(ensure(S.pvx, verts));
  HIPCHK(ensure(S.pvy, verts));
  if (int rc = launch(CmpOut{S.poff.p, S.pvx.p, S.pvy.p})) return rc;
  HIPCHK(hipMemcpyAsync(K.off.data(), S.poff.p, rows * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(K.px.data(), S.pvx.p, verts * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(K.py.data(), S.pvy.p, verts * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

// A route: which kernels carry the passes of a row kind (PointRows, PolygonRows: teb_costmap_host.hpp), where the write pass puts its
// rows, how the tables are installed. The single scene: the by-value kernels on the one record of the handle's costmap; its table is
// the handle's; no via-points.
struct OneSceneRoute {
  const int32_t* via_count = nullptr;
  const double *via_x = nullptr, *via_y = nullptr;
  bool rows_live = false;   // the write pass filled the rows of the live table itself

  int count(teb_amd_handle* h, PointRows& K) {
    auto& S = h->cmx;
    const CmoSceneRec& q = K.rec[0];
    const size_t lanes = K.max_lanes;
    if (lanes == 0) return TEB_AMD_OK;
    HIPCHK(ensure(S.cnt, lanes + 1));
    LAUNCH(costmap_obstacles_count_kernel, dim3((unsigned)((lanes + kCmoThreads - 1) / kCmoThreads)), dim3(kCmoThreads), 0, h->stream, q.g, q.f, q.ncols,
           q.nrows, q.chunk, q.nchunks, S.cnt.p);
    LAUNCH(costmap_obstacles_scan_kernel, dim3(1), dim3(kCmoScanThreads), 0, h->stream, S.cnt.p, (int)lanes);
    HIPCHK(hipMemcpyAsync(&K.tot[0], S.cnt.p + lanes, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return synced(h);
  }
  // the cell rows straight into the live table (they are known to fit), the custom rows behind them from the host; only the centres
  // come back, for the host copy and the out arrays
  int write(teb_amd_handle* h, PointRows& K, const SceneInputs& in) {
    const CmoSceneRec& q = K.rec[0];
    const size_t n = K.rows;
    if (n > 0)
      LAUNCH(costmap_obstacles_write_kernel, dim3((unsigned)((K.max_lanes + kCmoThreads - 1) / kCmoThreads)), dim3(kCmoThreads), 0, h->stream, q.g, q.f,
             q.ncols, q.nrows, q.chunk, q.nchunks, h->cmx.cnt.p, h->scene.rows());
    if (int rc = upload_obstacle_rows(h, in.tabs[0], n)) return rc;   // (ends in a stream synchronisation)
    rows_live = true;
    if (n == 0) return TEB_AMD_OK;
    HIPCHK(hipMemcpyAsync(K.px.data(), h->scene.ax.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(K.py.data(), h->scene.ay.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return synced(h);
  }
  // count + a scan over blocks per total; the host reads the three totals back
  int count(teb_amd_handle* h, PolygonRows& K) {
    auto& S = h->cmx;
    const CmpSceneRec& r = K.rec[0];
    if (r.nblk == 0) return TEB_AMD_OK;
    HIPCHK(ensure(S.pcnt, 3 * ((size_t)r.nblk + 1)));
    LAUNCH(costmap_polygons_count_kernel, dim3((unsigned)r.nblk), dim3(kCmpThreads), 0, h->stream, r.g, r.f, r.q, r.nblk, S.pcnt.p);
    for (int a = 0; a < 3; ++a) {
      int* c = S.pcnt.p + (size_t)a * (r.nblk + 1);
      LAUNCH(costmap_obstacles_scan_kernel, dim3(1), dim3(kCmoScanThreads), 0, h->stream, c, r.nblk);
      HIPCHK(hipMemcpyAsync(&K.tot[a], c + r.nblk, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    }
    return synced(h);
  }
  int write(teb_amd_handle* h, PolygonRows& K, const SceneInputs&) {
    const CmpSceneRec& r = K.rec[0];
    return write_polygon_rows(h, K, [&](const CmpOut& o) -> int {
      LAUNCH(costmap_polygons_write_kernel, dim3((unsigned)r.nblk), dim3(kCmpThreads), 0, h->stream, r.g, r.f, r.q, r.nblk, h->cmx.pcnt.p, o);
      return TEB_AMD_OK;
    });
  }
  int install(teb_amd_handle* h, std::vector<HostObst>&& tabs, SceneInputs&&) {
    if (!rows_live)
      if (int rc = upload_obstacle_rows(h, tabs[0], 0)) return rc;
    return install_obstacles(h, std::move(tabs[0]));
  }
};

// The scenes of a set over the grids of the costmap set: the records of the scenes on the device, every pass ONE launch of the
// record-reading kernels, one copy of the totals, one read-back; the tables become the scene set of the handle. The records travel
// before the count pass and again before the write pass: they carry the prefixes then.
struct SceneSetRoute {
  const int32_t* via_count;
  const double *via_x, *via_y;

  int count(teb_amd_handle* h, PointRows& K) {
    auto& S = h->cmx;
    const unsigned n = (unsigned)K.rec.size(), blocks = (unsigned)((K.max_lanes + kCmoThreads - 1) / kCmoThreads);
    HIPCHK(ensure(S.cnt, K.counters));
    HIPCHK(ensure(S.rec, (size_t)h->max_tebs));
    HIPCHK(ensure(S.tot, (size_t)h->max_tebs));
    HIPCHK(hipMemcpyAsync(S.rec.p, K.rec.data(), n * sizeof(CmoSceneRec), hipMemcpyHostToDevice, h->stream));
    if (blocks > 0) LAUNCH(costmap_obstacles_count_fleet_kernel, dim3(blocks, n), dim3(kCmoThreads), 0, h->stream, S.rec.p, S.cnt.p);
    LAUNCH(costmap_obstacles_scan_fleet_kernel, dim3(n), dim3(kCmoScanThreads), 0, h->stream, S.rec.p, S.cnt.p, S.tot.p);
    HIPCHK(hipMemcpyAsync(K.tot.data(), S.tot.p, n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return synced(h);
  }
  // every scene's points at its prefix offset of one scratch buffer
  int write(teb_amd_handle* h, PointRows& K, const SceneInputs&) {
    auto& S = h->cmx;
    const unsigned n = (unsigned)K.rec.size(), blocks = (unsigned)((K.max_lanes + kCmoThreads - 1) / kCmoThreads);
    if (K.rows == 0) return TEB_AMD_OK;
    HIPCHK(ensure(S.px, (size_t)std::max(h->max_obst, 1)));
    HIPCHK(ensure(S.py, (size_t)std::max(h->max_obst, 1)));
    HIPCHK(hipMemcpyAsync(S.rec.p, K.rec.data(), n * sizeof(CmoSceneRec), hipMemcpyHostToDevice, h->stream));
    LAUNCH(costmap_obstacles_write_fleet_kernel, dim3(blocks, n), dim3(kCmoThreads), 0, h->stream, S.rec.p, S.cnt.p, S.px.p, S.py.p);
    HIPCHK(hipMemcpyAsync(K.px.data(), S.px.p, K.rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(K.py.data(), S.py.p, K.rows * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return synced(h);
  }
  int count(teb_amd_handle* h, PolygonRows& K) {
    auto& S = h->cmx;
    const unsigned n = (unsigned)K.rec.size();
    HIPCHK(ensure(S.pcnt, 3 * (size_t)K.ncnt));
    HIPCHK(ensure(S.prec, (size_t)h->max_tebs));
    HIPCHK(ensure(S.blk, (size_t)h->max_tebs + 1));
    HIPCHK(ensure(S.ptot, 3 * (size_t)h->max_tebs));
    HIPCHK(hipMemcpyAsync(S.prec.p, K.rec.data(), n * sizeof(CmpSceneRec), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(S.blk.p, K.blk0.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (K.blocks > 0)
      LAUNCH(costmap_polygons_count_fleet_kernel, dim3((unsigned)K.blocks), dim3(kCmpThreads), 0, h->stream, S.prec.p, S.blk.p, (int)n, (int)K.ncnt, S.pcnt.p);
    LAUNCH(costmap_polygons_scan_fleet_kernel, dim3(3 * n), dim3(kCmoScanThreads), 0, h->stream, S.prec.p, (int)n, (int)K.ncnt, S.pcnt.p, S.ptot.p);
    HIPCHK(hipMemcpyAsync(K.tot.data(), S.ptot.p, K.tot.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    return synced(h);
  }
  int write(teb_amd_handle* h, PolygonRows& K, const SceneInputs&) {
    auto& S = h->cmx;
    const int n = (int)K.rec.size();
    return write_polygon_rows(h, K, [&](const CmpOut& o) -> int {
      HIPCHK(hipMemcpyAsync(S.prec.p, K.rec.data(), (size_t)n * sizeof(CmpSceneRec), hipMemcpyHostToDevice, h->stream));
      LAUNCH(costmap_polygons_write_fleet_kernel, dim3((unsigned)K.blocks), dim3(kCmpThreads), 0, h->stream, S.prec.p, S.blk.p, n, (int)K.ncnt, S.pcnt.p, o);
      return TEB_AMD_OK;
    });
  }
  int install(teb_amd_handle* h, std::vector<HostObst>&& tabs, SceneInputs&& in) {
    return install_scene_set(h, std::move(tabs), std::move(in.vc), via_x, via_y, in.vias);
  }
};

// The conversion, after the entry point's own argument checks (step 1 of 7). grids / poses / tiles: one per scene; custom: the caller's
// tables (null: none), which with the route's via-points may hold at most `early` - what a call checks only together with its
// converted rows is SIZE_MAX there. Nothing live is touched before the converted rows are known to fit.
extern "C++" template <class Rows, class Route>
int convert_costmaps(teb_amd_handle* h, const char* fn, Route route, const GridDev* grids, int n, const double* poses, double behind_robot_dist,
                     const int32_t* tiles, const teb_amd_obstacles_t* custom, const SceneCaps& early, const typename Rows::Out& out) {
  SceneInputs in;                                                                             // 2. the caller's tables and via-points
  if (Refusal r = parse_scene_inputs(n, custom, "bad custom obstacle table", route.via_count, route.via_x, route.via_y, early, in)) return fail(r.code, r.text);
  Rows K;                                                                                     // 3. the launch geometry per grid
  if (Refusal r = K.layout(grids, n, poses, behind_robot_dist, tiles)) return fail(r.code, std::string(fn) + r.text);
  if (int rc = route.count(h, K)) return rc;                                                  // 4. count + scan into scratch, totals back
  if (Refusal r = K.place(in, handle_caps(h), out)) return fail(r.code, r.text);              // 5. counts reported; refused if they do not fit
  if (int rc = route.write(h, K, in)) return rc;                                              // 6. the write pass and its read-back
  std::vector<HostObst> tabs;                                                                 // 7. host tables, out arrays, install
  if (const char* bad = K.finish(in, out, tabs)) return fail(TEB_AMD_ERR_INVALID_ARG, bad);
  return route.install(h, std::move(tabs), std::move(in));
}
}  // namespace

int teb_amd_set_obstacles_from_costmap(teb_amd_handle_t* h, const double* robot_pose, double costmap_obstacles_behind_robot_dist,
                                       const teb_amd_obstacles_t* custom, int32_t* n_costmap, double* out_x, double* out_y,
                                       int32_t capacity) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = refuse_in_fleet_mode(h, "teb_amd_set_obstacles_from_costmap")) return rc;
  const char* fn = "teb_amd_set_obstacles_from_costmap: ";
  if (h->cm.sx <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "no costmap (teb_amd_set_costmap)");
  if (!robot_pose || capacity < 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "null pose / negative capacity");
  // Early, before any launch: only the custom polygon vertices against max_obstacle_vertices - the point route adds none. The custom
  // rows are checked after the count pass, together with the cells (one refusal, n_costmap written before it).
  return convert_costmaps<PointRows>(h, fn, OneSceneRoute{}, &h->cm, 1, robot_pose, costmap_obstacles_behind_robot_dist, nullptr, custom,
                                     SceneCaps{SIZE_MAX, (size_t)h->max_verts, SIZE_MAX}, PointRows::Out{n_costmap, out_x, out_y, capacity});
}

int teb_amd_set_obstacles_from_costmap_polygons(teb_amd_handle_t* h, const double* robot_pose, double costmap_obstacles_behind_robot_dist,
                                                int32_t tile_cells, const teb_amd_obstacles_t* custom, int32_t* n_obstacles,
                                                int32_t* n_points, int32_t* out_offset, double* out_x, double* out_y,
                                                int32_t capacity_obstacles, int32_t capacity_points) {
  if (int rc = check_handle(h)) return rc;
  if (int rc = refuse_in_fleet_mode(h, "teb_amd_set_obstacles_from_costmap_polygons")) return rc;
  const char* fn = "teb_amd_set_obstacles_from_costmap_polygons: ";
  if (h->cm.sx <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "no costmap (teb_amd_set_costmap)");
  if (!robot_pose || capacity_obstacles < 0 || capacity_points < 0)
    return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "null pose / negative capacity");
  if (tile_cells < 1 || tile_cells > kCmpMaxTile) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "tile_cells outside 1 .. 64");
  // Early, before any launch: nothing. Custom rows and custom polygon vertices are both checked after the count pass, each together
  // with the converted ones (n_obstacles / n_points written before either refusal).
  return convert_costmaps<PolygonRows>(h, fn, OneSceneRoute{}, &h->cm, 1, robot_pose, costmap_obstacles_behind_robot_dist, &tile_cells, custom, SceneCaps{},
                                       PolygonRows::Out{n_obstacles, n_points, out_offset, out_x, out_y, capacity_obstacles, capacity_points});
}

int teb_amd_set_scenes_from_costmaps(teb_amd_handle_t* h, int32_t n_scenes, const double* robot_pose, double costmap_obstacles_behind_robot_dist,
                                     const teb_amd_obstacles_t* custom, const int32_t* via_count, const double* via_x, const double* via_y,
                                     int32_t* n_costmap, double* out_x, double* out_y, int32_t capacity) {
  if (int rc = check_handle(h)) return rc;
  const char* fn = "teb_amd_set_scenes_from_costmaps: ";
  if (n_scenes < 1 || !robot_pose || capacity < 0)
    return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "needs at least one scene, the robot poses and a capacity >= 0");
  if (h->cms.n != n_scenes) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "needs a costmap set with one grid per scene (teb_amd_set_costmaps)");
  // Early, as teb_amd_set_scenes: custom rows, custom polygon vertices and via-points each against the handle's capacity; after the
  // count pass the rows again, together with the cells.
  return convert_costmaps<PointRows>(h, fn, SceneSetRoute{via_count, via_x, via_y}, h->cms.grids_host.data(), n_scenes, robot_pose,
                                     costmap_obstacles_behind_robot_dist, nullptr, custom, handle_caps(h), PointRows::Out{n_costmap, out_x, out_y, capacity});
}

// teb_amd_set_scenes_from_costmaps on the polygon route: every scene's grid at the scene's own tile size
int teb_amd_set_scenes_from_costmap_polygons(teb_amd_handle_t* h, int32_t n_scenes, const double* robot_pose, double costmap_obstacles_behind_robot_dist,
                                             const int32_t* tile_cells, const teb_amd_obstacles_t* custom, const int32_t* via_count, const double* via_x,
                                             const double* via_y, int32_t* n_obstacles, int32_t* n_points, int32_t* out_offset, double* out_x,
                                             double* out_y, int32_t capacity_obstacles, int32_t capacity_points) {
  if (int rc = check_handle(h)) return rc;
  const char* fn = "teb_amd_set_scenes_from_costmap_polygons: ";
  if (n_scenes < 1 || !robot_pose || !tile_cells || capacity_obstacles < 0 || capacity_points < 0)
    return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "needs at least one scene, the robot poses, the tile sizes and capacities >= 0");
  if (h->cms.n != n_scenes) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "needs a costmap set with one grid per scene (teb_amd_set_costmaps)");
  for (int s = 0; s < n_scenes; ++s)
    if (tile_cells[s] < 1 || tile_cells[s] > kCmpMaxTile) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "tile_cells outside 1 .. 64");
  // Early, as teb_amd_set_scenes: all three capacities; after the count pass rows and polygon vertices again, with the converted ones.
  return convert_costmaps<PolygonRows>(h, fn, SceneSetRoute{via_count, via_x, via_y}, h->cms.grids_host.data(), n_scenes, robot_pose,
                                       costmap_obstacles_behind_robot_dist, tile_cells, custom, handle_caps(h),
                                       PolygonRows::Out{n_obstacles, n_points, out_offset, out_x, out_y, capacity_obstacles, capacity_points});
}

namespace {
// bands[s] is a band of scene s, or negative
int check_feasibility_bands(const teb_amd_handle* h, const char* fn, const int32_t* bands) {
  for (int s = 0; s < h->fleet.n_scenes; ++s)
    if (bands[s] >= 0 && (bands[s] >= h->B || h->fleet.band_scene[bands[s]] != s)) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "%s: bands[%d] = %d is not a band of scene %d", fn, s, bands[s], s);
      return fail(TEB_AMD_ERR_INVALID_ARG, buf);
    }
  return TEB_AMD_OK;
}
}  // namespace

int teb_amd_is_trajectory_feasible_per_scene(teb_amd_handle_t* h, const int32_t* bands, int32_t nf, const double* fx, const double* fy,
                                             double inscribed_radius, double min_res_angular, int32_t look_ahead_idx, double lookahead_distance,
                                             int32_t* feasible, int32_t* first_infeasible) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_is_trajectory_feasible_per_scene"))) return rc;
  const int ns = h->fleet.n_scenes;
  if (h->cms.n != ns) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_is_trajectory_feasible_per_scene: needs a costmap set with one grid per scene (teb_amd_set_costmaps)");
  if ((rc = check_feasibility_arguments(bands && feasible && nf >= 1 && nf <= kMaxFeasFootprint && fx && fy, "bad bands / footprint / output", inscribed_radius, min_res_angular))) return rc;
  if ((rc = check_feasibility_bands(h, "teb_amd_is_trajectory_feasible_per_scene", bands))) return rc;
  return run_feasibility(h, ns, nf, fx, fy, feasible, first_infeasible, [&](double* px, double* py, int* fe, int* fi, int* ovf) {
    if (!h->cms_bands.p) HIPCHK(h->cms_bands.alloc((size_t)h->max_tebs));
    HIPCHK(hipMemcpyAsync(h->cms_bands.p, bands, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
    LAUNCH(feasibility_fleet_kernel, dim3(ns), dim3(kFeasThreads), 0, h->stream, h->bands.strips.n.p, h->bands.strips.x.p, h->bands.strips.y.p, h->bands.strips.th.p, h->stride, h->cms_bands.p, h->cms.grids.p, nf,
           px, py, inscribed_radius, min_res_angular, look_ahead_idx, lookahead_distance, 1 << 22, fe, fi, ovf);
    return (int)TEB_AMD_OK;
  });
}

int teb_amd_is_trajectory_feasible_per_class(teb_amd_handle_t* h, const int32_t* bands, int32_t n_specs, const teb_amd_feasibility_spec_t* specs,
                                             const int32_t* spec_of_scene, int32_t* feasible, int32_t* first_infeasible) {
  int rc = check_handle(h);
  if (rc) return rc;
  const char* fn = "teb_amd_is_trajectory_feasible_per_class";
  if ((rc = require_fleet_mode(h, fn))) return rc;
  const int ns = h->fleet.n_scenes;
  if (h->cms.n != ns) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + ": needs a costmap set with one grid per scene (teb_amd_set_costmaps)");
  if (!bands || !feasible) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + ": bad bands / output");
  const ClassList cl = fleet_classes(h);
  const FeasibilitySpecs fs = check_feasibility_specs(specs, n_specs, spec_of_scene, ns, cl.n, kMaxFeasFootprint);
  if (!fs.refusal.ok()) {
    char buf[240];
    if (fs.refusal.spec >= 0) std::snprintf(buf, sizeof buf, "%s: spec %d: %s", fn, fs.refusal.spec, fs.refusal.why);
    else if (fs.refusal.scene >= 0) std::snprintf(buf, sizeof buf, "%s: spec_of_scene[%d] = %d with %d specs: %s", fn, fs.refusal.scene, spec_of_scene[fs.refusal.scene], n_specs, fs.refusal.why);
    else std::snprintf(buf, sizeof buf, "%s: %d specs, %d classes: %s", fn, n_specs, cl.n, fs.refusal.why);
    return fail(TEB_AMD_ERR_INVALID_ARG, buf);
  }
  if ((rc = check_feasibility_bands(h, fn, bands))) return rc;
  // the footprints of all specs one after the other (x plane, y plane), and the record of every scene
  const int total = fs.offset.back();
  std::vector<double> fx((size_t)total), fy((size_t)total);
  for (int k = 0; k < n_specs; ++k) {
    std::copy(specs[k].footprint_x, specs[k].footprint_x + specs[k].n_footprint, fx.begin() + fs.offset[k]);
    std::copy(specs[k].footprint_y, specs[k].footprint_y + specs[k].n_footprint, fy.begin() + fs.offset[k]);
  }
  std::vector<FeasSpecDev> recs((size_t)ns);
  for (int s = 0; s < ns; ++s) {
    const int k = feasibility_spec_of(spec_of_scene, cl.class_of, s);
    const teb_amd_feasibility_spec_t& q = specs[k];
    recs[s] = FeasSpecDev{fs.offset[k], q.n_footprint, q.inscribed_radius, q.min_resolution_collision_check_angular, q.look_ahead_idx,
                          q.feasibility_check_lookahead_distance};
  }
  return run_feasibility(h, ns, total, fx.data(), fy.data(), feasible, first_infeasible, [&](double* px, double* py, int* fe, int* fi, int* ovf) {
    if (!h->cms_bands.p) HIPCHK(h->cms_bands.alloc((size_t)h->max_tebs));
    if (!h->cms_specs.p) HIPCHK(h->cms_specs.alloc((size_t)h->max_tebs));
    HIPCHK(hipMemcpyAsync(h->cms_bands.p, bands, (size_t)ns * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->cms_specs.p, recs.data(), (size_t)ns * sizeof(FeasSpecDev), hipMemcpyHostToDevice, h->stream));
    LAUNCH(feasibility_fleet_class_kernel, dim3(ns), dim3(kFeasThreads), 0, h->stream, h->bands.strips.n.p, h->bands.strips.x.p, h->bands.strips.y.p,
           h->bands.strips.th.p, h->stride, h->cms_bands.p, h->cms.grids.p, h->cms_specs.p, px, py, 1 << 22, fe, fi, ovf);
    return (int)TEB_AMD_OK;
  });
}

namespace {
// teb_amd_update_and_prune_per_scene (min_samples: the one value of the call) and teb_amd_update_and_prune_per_class (null: the eleventh
// column of the message, min_samples of every scene's class)
int update_and_prune_fleet(teb_amd_handle* h, const char* fn, const double* new_start, const double* new_goal, const int32_t* min_samples,
                           const double* start_vel, const int32_t* has_start_vel) {
  int rc = TEB_AMD_OK;
  if ((rc = require_fleet_mode(h, fn))) return rc;
  if (h->B <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "no TEBs on the device");
  if ((rc = check_band_scenes(h, h->B))) return rc;
  const size_t ns = (size_t)h->fleet.n_scenes;
  // one message: [start | goal | start_vel] 3 ns each, [has_start_vel] ns, [min_samples] ns (exact as doubles)
  std::vector<double> msg(11 * ns, 0.0);
  if (new_start) std::copy(new_start, new_start + 3 * ns, msg.begin());
  if (new_goal) std::copy(new_goal, new_goal + 3 * ns, msg.begin() + 3 * ns);
  if (start_vel) {
    std::copy(start_vel, start_vel + 3 * ns, msg.begin() + 6 * ns);
    for (size_t s = 0; s < ns; ++s) msg[9 * ns + s] = (!has_start_vel || has_start_vel[s]) ? 1.0 : 0.0;
  }
  if (!min_samples) {
    const ClassList cl = fleet_classes(h);
    for (size_t s = 0; s < ns; ++s) msg[10 * ns + s] = (double)scene_tick_params(cl.cfgs, cl.n, cl.class_of, (int)s).min_samples;
  }
  if (!h->prune_msg.p) HIPCHK(h->prune_msg.alloc(11 * (size_t)h->max_tebs));
  HIPCHK(hipMemcpyAsync(h->prune_msg.p, msg.data(), msg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));   // the upload reads msg; nothing waits for the kernel
  LAUNCH(prune_fleet_kernel, dim3(h->B), dim3(kThreads), 4 * (size_t)h->stride * sizeof(double), h->stream, batch_of(h), h->fleet.scene_of.p, h->prune_msg.p,
         (int)ns, new_start ? 1 : 0, new_goal ? 1 : 0, start_vel ? 1 : 0, min_samples ? *min_samples : 0, min_samples ? 0 : 1, h->bands.has_vs.p, h->bands.vs.p);
  h->bands_changed();
  return TEB_AMD_OK;
}
}  // namespace

int teb_amd_update_and_prune_per_scene(teb_amd_handle_t* h, const double* new_start, const double* new_goal, int32_t min_samples,
                                       const double* start_vel, const int32_t* has_start_vel) {
  if (int rc = check_handle(h)) return rc;
  return update_and_prune_fleet(h, "teb_amd_update_and_prune_per_scene", new_start, new_goal, &min_samples, start_vel, has_start_vel);
}

int teb_amd_update_and_prune_per_class(teb_amd_handle_t* h, const double* new_start, const double* new_goal, const double* start_vel,
                                       const int32_t* has_start_vel) {
  if (int rc = check_handle(h)) return rc;
  return update_and_prune_fleet(h, "teb_amd_update_and_prune_per_class", new_start, new_goal, nullptr, start_vel, has_start_vel);
}

int teb_amd_get_velocity_commands(teb_amd_handle_t* h, int32_t n, const int32_t* bands, int32_t look_ahead_poses,
                                  int32_t prevent_look_ahead_poses_near_goal, double* cmd, int32_t* ok) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!bands || !cmd || !ok))) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_get_velocity_commands: bad arguments");
  bool any = false;
  for (int i = 0; i < n; ++i) {
    if (bands[i] >= h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
    any = any || bands[i] >= 0;
  }
  std::vector<double> c;
  if (any) {
    if ((rc = run_consumers(h, look_ahead_poses, prevent_look_ahead_poses_near_goal))) return rc;
    c.resize(4 * (size_t)h->B);
    HIPCHK(hipMemcpyAsync(c.data(), h->out_cmd.p, c.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  for (int i = 0; i < n; ++i) {
    const double* q = bands[i] >= 0 ? c.data() + 4 * (size_t)bands[i] : nullptr;
    cmd[3 * i] = q ? q[0] : 0.0; cmd[3 * i + 1] = q ? q[1] : 0.0; cmd[3 * i + 2] = q ? q[2] : 0.0;
    ok[i] = q ? q[3] != 0 : 0;
  }
  return TEB_AMD_OK;
}

// ---- local plan windows per robot from resident global plans (teb_amd.h; kernel in teb_plan_window.hpp) ----------------------------
void teb_amd_plan_window_params_default(teb_amd_plan_window_params_t* p) {   // teb_config.h:261-264; moving_average_length: teb_local_planner_ros.h
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->struct_size = (int32_t)sizeof(*p);
  p->global_plan_prune_distance = 1; p->max_global_plan_lookahead_dist = 1; p->global_plan_viapoint_sep = -1;
  p->global_plan_overwrite_orientation = 1; p->moving_average_length = 3;
}
int teb_amd_sizeof_plan_window_params(void) { return (int)sizeof(teb_amd_plan_window_params_t); }

int teb_amd_set_global_plans(teb_amd_handle_t* h, int32_t n, const int32_t* plan_count, const double* x, const double* y, const double* yaw,
                             const int32_t* begin) {
  int rc = check_handle(h);
  if (rc) return rc;
  auto& P = h->plans;
  const char* fn = "teb_amd_set_global_plans: ";
  if (n < 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "negative number of plans");
  if (n == 0) { P.n = 0; P.total = 0; P.count_host.clear(); return TEB_AMD_OK; }
  if (n > h->max_tebs) return fail(TEB_AMD_ERR_CAPACITY, std::string(fn) + "more plans than max_tebs");
  if (!plan_count) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "null plan_count");
  // everything is checked before the first upload: on a bad argument the previous set stays
  std::vector<long long> first(n);
  std::vector<int> cur(n, 0);
  size_t total = 0;
  for (int r = 0; r < n; ++r) {
    if (plan_count[r] < 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "negative pose count");
    if (begin && (begin[r] < 0 || begin[r] > plan_count[r])) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "cursor outside 0 .. count");
    first[r] = (long long)total;
    total += (size_t)plan_count[r];
    if (begin) cur[r] = begin[r];
  }
  if (total > 0 && (!x || !y || !yaw)) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "null pose array");
  // The per-robot buffers of the first call, all six or none: a failed allocation leaves its buffer empty, so a later call comes here
  // again and allocates each over what it holds (no previous set exists yet at that point).
  if (!P.first.p || !P.count.p || !P.cursor.p || !P.rec.p || !P.in.p || !P.ticket.p) {
    const size_t T = (size_t)h->max_tebs;
    if (P.first.alloc(T) != hipSuccess || P.count.alloc(T) != hipSuccess || P.cursor.alloc(T) != hipSuccess || P.rec.alloc(T) != hipSuccess ||
        P.in.alloc(9 * T) != hipSuccess || P.ticket.alloc(1) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TEB_AMD_ERR_HIP, std::string(fn) + "device allocation failed");
    }
  }
  // the new buffers before the old ones go: a failed allocation leaves the previous set. A window holds at most the poses of its plan
  // and the inserted start, so 5 (total + n) doubles hold the windows and via-points of every robot (PlanWinOut::alloc).
  if (P.poses.n < 3 * total || P.pack.n < 5 * (total + (size_t)h->max_tebs)) {
    DevBuf<double> np, nk;
    if (np.alloc(3 * total) != hipSuccess || nk.alloc(5 * (total + (size_t)h->max_tebs)) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TEB_AMD_ERR_HIP, std::string(fn) + "device allocation failed");
    }
    P.poses = std::move(np); P.pack = std::move(nk);
  }
  P.n = 0;   // from here on the previous plans are overwritten: a HIP error leaves no set
  P.count_host.clear();
  HIPCHK(upload(h->stream, P.poses.p, x, total));
  HIPCHK(upload(h->stream, P.poses.p + total, y, total));
  HIPCHK(upload(h->stream, P.poses.p + 2 * total, yaw, total));
  HIPCHK(upload(h->stream, P.first.p, first.data(), (size_t)n));
  HIPCHK(upload(h->stream, P.count.p, plan_count, (size_t)n));
  HIPCHK(upload(h->stream, P.cursor.p, cur.data(), (size_t)n));
  HIPCHK(hipStreamSynchronize(h->stream));   // the caller's buffers may go away
  P.count_host.assign(plan_count, plan_count + n);
  P.total = total;
  P.n = n;
  return TEB_AMD_OK;
}

int teb_amd_get_plan_cursors(teb_amd_handle_t* h, int32_t* begin) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (h->plans.n == 0) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_get_plan_cursors: no global plans set (teb_amd_set_global_plans)");
  if (!begin) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_get_plan_cursors: null argument");
  HIPCHK(hipMemcpyAsync(begin, h->plans.cursor.p, (size_t)h->plans.n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

int teb_amd_plan_windows(teb_amd_handle_t* h, int32_t n, const teb_amd_plan_window_params_t* params, const double* robot_pose,
                         const double* plan_to_global, const double* dist_threshold, int32_t* window_count, int32_t* goal_idx,
                         int32_t* cursor, int32_t* pruned, double* goal, double* global_goal, int32_t* via_count, int32_t* offset,
                         double* win_x, double* win_y, double* win_yaw, int32_t capacity_window, int32_t* via_offset, double* via_x,
                         double* via_y, int32_t capacity_via) {
  int rc = check_handle(h);
  if (rc) return rc;
  auto& P = h->plans;
  const char* fn = "teb_amd_plan_windows: ";
  if (P.n == 0) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "no global plans set (teb_amd_set_global_plans)");
  if (n != P.n) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "the plan set holds another number of robots");
  if (!robot_pose || !dist_threshold || capacity_window < 0 || capacity_via < 0)
    return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "needs the robot poses, the distance thresholds and capacities >= 0");
  teb_amd_plan_window_params_t prm;
  teb_amd_plan_window_params_default(&prm);
  if (params) {
    if (params->struct_size != (int32_t)sizeof(prm)) return fail(TEB_AMD_ERR_INVALID_ARG, std::string(fn) + "params of another struct_size");
    prm = *params;
  }
  const size_t N = (size_t)n;
  // one upload of what changes per tick: poses [3 n] | thresholds [n] | transforms [5 n]
  std::vector<double> in(9 * N);
  std::copy(robot_pose, robot_pose + 3 * N, in.begin());
  std::copy(dist_threshold, dist_threshold + N, in.begin() + 3 * N);
  if (plan_to_global) std::copy(plan_to_global, plan_to_global + 5 * N, in.begin() + 4 * N);
  HIPCHK(upload(h->stream, P.in.p, in.data(), plan_to_global ? 9 * N : 4 * N));
  HIPCHK(hipMemsetAsync(P.ticket.p, 0, sizeof(unsigned long long), h->stream));
  PlanWinArgs a;
  a.px = P.poses.p; a.py = P.poses.p + P.total; a.pyaw = P.poses.p + 2 * P.total;
  a.first = P.first.p; a.count = P.count.p; a.cursor = P.cursor.p;
  a.pose = P.in.p; a.thr = P.in.p + 3 * N; a.tf = plan_to_global ? P.in.p + 4 * N : nullptr;
  a.prune_distance = prm.global_plan_prune_distance; a.max_plan_length = prm.max_global_plan_lookahead_dist;
  a.via_sep = prm.global_plan_viapoint_sep;
  a.overwrite_orientation = prm.global_plan_overwrite_orientation; a.moving_average_length = prm.moving_average_length;
  a.out = P.rec.p; a.pack = P.pack.p; a.ticket = P.ticket.p; a.pack_capacity = (long long)P.pack.n;
  LAUNCH(plan_window_kernel, dim3((unsigned)n), dim3(kPwThreads), 0, h->stream, a);
  std::vector<PlanWinOut> rec(N);
  HIPCHK(hipMemcpyAsync(rec.data(), P.rec.p, N * sizeof(PlanWinOut), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  // offset bookkeeping: the per-robot values, the offsets of the concatenations, what the pack buffer holds
  long long nw = 0, nv = 0, used = 0;
  for (size_t r = 0; r < N; ++r) {
    const PlanWinOut& q = rec[r];
    if (q.window_count > 0 && (q.off < 0 || q.off + 5ll * q.alloc > (long long)P.pack.n || q.window_count > q.alloc || q.via_count > q.alloc))
      return fail(TEB_AMD_ERR_HIP, std::string(fn) + "a window left its block of the pack buffer");
    if (window_count) window_count[r] = q.window_count;
    if (goal_idx) goal_idx[r] = q.goal_idx;
    if (cursor) cursor[r] = q.cursor;
    if (pruned) pruned[r] = q.pruned;
    if (via_count) via_count[r] = q.via_count;
    if (goal) std::copy(q.goal, q.goal + 3, goal + 3 * r);
    if (global_goal) std::copy(q.global_goal, q.global_goal + 3, global_goal + 3 * r);
    if (offset) offset[r] = (int32_t)nw;
    if (via_offset) via_offset[r] = (int32_t)nv;
    nw += q.window_count; nv += q.via_count;
    if (q.window_count > 0) used = std::max(used, q.off + 5ll * q.alloc);
  }
  if (nw > std::numeric_limits<int32_t>::max()) return fail(TEB_AMD_ERR_CAPACITY, std::string(fn) + "more window poses than an offset holds");
  if (offset) offset[N] = (int32_t)nw;
  if (via_offset) via_offset[N] = (int32_t)nv;
  const bool want_win = win_x || win_y || win_yaw, want_via = via_x || via_y;
  const bool win_fits = nw <= capacity_window, via_fits = nv <= capacity_via;
  if ((want_win && win_fits && nw > 0) || (want_via && via_fits && nv > 0)) {
    std::vector<double> pack((size_t)used);
    HIPCHK(hipMemcpyAsync(pack.data(), P.pack.p, (size_t)used * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    long long iw = 0, iv = 0;
    for (size_t r = 0; r < N; ++r) {
      const PlanWinOut& q = rec[r];
      if (q.window_count > 0) {
        const double* b = pack.data() + q.off;
        const size_t A = (size_t)q.alloc, W = (size_t)q.window_count, V = (size_t)q.via_count;
        if (want_win && win_fits) {
          if (win_x) std::copy(b, b + W, win_x + iw);
          if (win_y) std::copy(b + A, b + A + W, win_y + iw);
          if (win_yaw) std::copy(b + 2 * A, b + 2 * A + W, win_yaw + iw);
        }
        if (want_via && via_fits) {
          if (via_x) std::copy(b + 3 * A, b + 3 * A + V, via_x + iv);
          if (via_y) std::copy(b + 4 * A, b + 4 * A + V, via_y + iv);
        }
      }
      iw += q.window_count; iv += q.via_count;
    }
  }
  if ((want_win && !win_fits) || (want_via && !via_fits))
    return fail(TEB_AMD_ERR_CAPACITY, std::string(fn) + "the windows or the via-points exceed the caller's arrays");
  return TEB_AMD_OK;
}

// ---- f3 (candidate generation): createGraph + DepthFirst + addAndInitNewTeb (kernels in teb_graph.hpp) ---------------------------
void teb_amd_hcp_params_default(teb_amd_hcp_params_t* p) {   // teb_config.h:352-367, :260, :293
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->simple_exploration = 0; p->roadmap_graph_no_samples = 15; p->roadmap_graph_area_width = 6; p->roadmap_graph_area_length_scale = 1.0;
  p->obstacle_heading_threshold = 0.45; p->xy_goal_tolerance = 0.2; p->max_number_classes = 5;
  p->max_number_plans_in_current_class = 1;   // no constructor default in the reference; 1 is its dynamic-reconfigure default
  p->h_signature_prescaler = 1; p->h_signature_threshold = 0.1; p->allow_init_with_backwards_motion = 0;
  p->delete_detours_backwards = 1; p->detours_orientation_tolerance = M_PI / 2.0; p->length_start_orientation_vector = 0.4;   // :374-377
  p->max_ratio_detours_duration_best_duration = 3.0;
  p->global_plan_overwrite_orientation = 1; p->viapoints_all_candidates = 1;   // :259, :370
}

namespace {
constexpr int kCandChunk = 64;   // candidate paths initialised and classified per device round trip

int ensure_candidate_buffers(teb_amd_handle* h) {
  if (h->cand.bands()) return TEB_AMD_OK;
  const size_t W = (size_t)(h->max_obst > 2 ? h->max_obst : 2);
  AllocRun A;
  A(h->cand_sig.alloc(std::max<size_t>(kCandChunk * W, 4 * (size_t)h->max_tebs)));   // signatures of a chunk / detour statistics of the batch
  A(h->cand_px.alloc((size_t)kCandChunk * (h->stride + 1)));
  A(h->cand_py.alloc((size_t)kCandChunk * (h->stride + 1))); A(h->cand_off.alloc(kCandChunk + 1)); A(h->cand_map.alloc(h->max_tebs));
  if (A.ok()) A(h->cand.alloc(kCandChunk, h->stride));   // last: the strips say that the scratch exists
  if (!A.ok()) return fail(TEB_AMD_ERR_HIP, "candidate scratch allocation failed");
  return TEB_AMD_OK;
}

constexpr int kExploreQuota = 16;  // paths a scene contributes to a round of a fleet (teb_amd_debug_set_explore_quota overrides it)

// the candidate scratch of the scene set, for K candidates and `values` signature values; grows, never shrinks
int ensure_fleet_candidate_buffers(teb_amd_handle* h, size_t K, size_t values) {
  auto& F = h->fleet;
  AllocRun A;
  if (F.ex.bands() < K) {
    const size_t KP = K * ((size_t)h->stride + 1);
    F.ex.free();   // (first: a failure below leaves no strips, so the next call comes here again)
    A(F.ex_px.alloc(KP)); A(F.ex_py.alloc(KP)); A(F.ex_pyaw.alloc(KP)); A(F.ex_off.alloc(K + 1)); A(F.ex_scene.alloc(K));
    A(F.ex_soff.alloc(K + 1)); A(F.ex_line.alloc(6 * K));
    if (A.ok()) A(F.ex.alloc(K, h->stride));
  }
  A(ensure(F.ex_sig, std::max<size_t>(values, 2)));
  A(ensure(F.ex_map, (size_t)h->max_tebs));
  if (F.ex_orient.n < 2 * (size_t)h->max_tebs) { A(F.ex_rec.alloc(h->max_tebs)); A(F.ex_orient.alloc(2 * (size_t)h->max_tebs)); }
  if (!A.ok()) { (void)hipGetLastError(); return fail(TEB_AMD_ERR_HIP, "teb_amd_explore_candidates_per_scene: candidate scratch allocation failed"); }
  return TEB_AMD_OK;
}

// ---- the exploration tick: exploreEquivalenceClassesAndInitTebs (src/homotopy_class_planner.cpp:337-384), getInitialPlanTEB and
// updateReferenceTrajectoryViaPoints, written once over a list of planners. The decisions are the host rules of teb_hcp_host.hpp; the
// device steps between them belong to a route: the single scene's kernels and scratch (SingleRoute, one planner) or the fleet forms
// (FleetRoute, one planner per scene). A route initialises candidates 0 .. who.size() - 1 of its scratch strips, candidate k for
// planner who[k], and computes their signatures; the candidates of a planner lie together.

// ONE planner of a tick
struct TickPlanner {
  const HostObst* tab = nullptr;   // its obstacle table
  PlannerMemory* mem = nullptr;
  ClassTable ct;                   // the classes of its bands, in band order
  std::vector<int> bands;          // its bands in the batch, in band order; grows with the accepted candidates
  const double *start = nullptr, *goal = nullptr, *start_vel = nullptr;   // [3] each; start_vel may be NULL
  int n_plan = 0; const double *plan_x = nullptr, *plan_y = nullptr, *plan_yaw = nullptr;   // the initial plan, n_plan <= 0: none
  const double* unit_samples = nullptr;   // [2 * roadmap_graph_no_samples] or NULL: drawn from mem->rnd
  int slots = 0, n_via = 0;        // most bands it may hold; its via-points
  double dist_to_obst = 0, weight_viapoint = 0;   // of its configuration: the graph's distance, the via-point rule of finish_tick
  int32_t *n_vertices = nullptr, *n_paths = nullptr, *initial_plan_teb = nullptr;   // output slots, NULL: not asked for
  // of the running tick
  int created = -1;                // initial_plan_teb_: the band made from the initial plan, as a position in `bands`
  std::vector<double> vx, vy;      // its graph; the adjacency matrix goes to mem->g_adj
  GraphArgs ga;                    // everything of the edge kernel's arguments but N, the vertex and the adjacency pointers
  PathSource paths;
  bool full() const { return (int)bands.size() >= slots; }   // src/graph_search.cpp:99-100, 231-232
};

// The scratch a route initialises its candidates in: strips seen as a batch, gather map, path points and their offsets, signatures
struct TickScratch { BatchDev cand; int *map, *off; double *px, *py, *sig; };

// tebs_.push_back(candidate) for the accepted candidates acc of a launch: bands of the scratch strips `cand` -> the next slots of the
// batch in one gather, with BandAttrs::candidate of their planner as arrays and, in a scene set, their entries of the band -> scene map
int append_candidates(teb_amd_handle* h, const TickScratch& sc, const std::vector<int>& acc, const std::vector<int>& who,
                      std::vector<TickPlanner>& P, int free_goal_vel) {
  if (acc.empty()) return TEB_AMD_OK;
  auto& F = h->fleet;
  const bool scene_map = F.n_scenes > 0;   // a scene set: planner s = scene s (the single scene keeps no map)
  const int slot0 = h->B, cnt = (int)acc.size();
  if (slot0 + cnt > h->max_tebs) return fail(TEB_AMD_ERR_CAPACITY, "more bands than max_tebs");   // (excluded by the slot limits)
  BandAttrArrays at((size_t)cnt);
  for (int k = 0; k < cnt; ++k) {
    TickPlanner& t = P[who[acc[k]]];
    at.set((size_t)k, BandAttrs::candidate(t.start_vel, free_goal_vel));
    if (scene_map) F.band_scene[slot0 + k] = who[acc[k]];
    t.bands.push_back(slot0 + k);
  }
  HIPCHK(hipMemcpyAsync(h->bands.has_vs.p + slot0, at.has_vs.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.has_vg.p + slot0, at.has_vg.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.rotdir.p + slot0, at.rotdir.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.via_en.p + slot0, at.via_en.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.optimized.p + slot0, at.optimized.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.vs.p + 3 * (size_t)slot0, at.vs.data(), at.vs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(h->bands.vg.p + 3 * (size_t)slot0, at.vg.data(), at.vg.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (scene_map) HIPCHK(hipMemcpyAsync(F.scene_of.p + slot0, F.band_scene.data() + slot0, cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(sc.map, acc.data(), cnt * sizeof(int), hipMemcpyHostToDevice, h->stream));
  h->B = slot0 + cnt;
  LAUNCH(move_bands_kernel, dim3(cnt), dim3(kThreads), 0, h->stream, sc.cand, batch_of(h), sc.map, slot0, 0);
  HIPCHK(hipStreamSynchronize(h->stream));   // the staging vectors live on this stack frame
  return TEB_AMD_OK;
}

// The single scene: one planner, candidates in chunks of kCandChunk through the cand_* scratch
struct SingleRoute {
  teb_amd_handle* h;
  const teb_amd_hcp_params_t* p;
  TickScratch sc;
  int per_round;
  int plans(std::vector<TickPlanner>& P, const std::vector<int>& who) {   // addAndInitNewTeb(*initial_plan_, ...), hcp.cpp:326-329, 412-440
    const TickPlanner& t = P[who[0]];
    if (int rc = stage(h, t.n_plan, t.plan_x, t.plan_y, t.plan_yaw)) return rc;
    hipLaunchKernelGGL(init_plan_kernel, dim3(1), dim3(kThreads), 0, h->stream, sc.cand, 0, t.n_plan, h->stage_x.p, h->stage_y.p, h->stage_yaw.p,
                       h->cfg.max_vel_x, h->cfg.max_vel_theta, p->global_plan_overwrite_orientation, h->cfg.min_samples,
                       p->allow_init_with_backwards_motion, h->err_flag.p);
    return TEB_AMD_OK;
  }
  int lines(std::vector<TickPlanner>& P, const std::vector<int>& who) {   // addAndInitNewTeb(start, goal, ...), hcp.cpp:358-384
    const TickPlanner& t = P[who[0]];
    HIPCHK(hipMemsetAsync(h->err_flag.p, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(init_line_kernel, dim3(1), dim3(kThreads), 0, h->stream, sc.cand, 0, t.start[0], t.start[1], t.start[2], t.goal[0], t.goal[1],
                       t.goal[2], 0.0, h->cfg.max_vel_x, h->cfg.min_samples, p->allow_init_with_backwards_motion, h->err_flag.p);
    return TEB_AMD_OK;
  }
  int edges(std::vector<TickPlanner>& P, const std::vector<int>& who) {
    TickPlanner& t = P[who[0]];
    const int N = (int)t.vx.size();
    if (h->g_vx.n < (size_t)N) { h->g_vx.free(); h->g_vy.free(); HIPCHK(h->g_vx.alloc(N)); HIPCHK(h->g_vy.alloc(N)); }
    if (h->g_adj.n < (size_t)N * N) { h->g_adj.free(); HIPCHK(h->g_adj.alloc((size_t)N * N)); }
    HIPCHK(hipMemcpyAsync(h->g_vx.p, t.vx.data(), N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->g_vy.p, t.vy.data(), N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    const long long pairs = (long long)N * N;
    t.ga.N = N; t.ga.gx = h->g_vx.p; t.ga.gy = h->g_vy.p; t.ga.adj = h->g_adj.p;
    LAUNCH(graph_edges_kernel, dim3((unsigned)((pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, h->stream, scene_of(h), t.ga);
    t.mem->g_adj.resize((size_t)pairs);
    HIPCHK(hipMemcpyAsync(t.mem->g_adj.data(), h->g_adj.p, (size_t)pairs, hipMemcpyDeviceToHost, h->stream));
    return synced(h);
  }
  int paths(std::vector<TickPlanner>& P, const std::vector<int>& who) {   // the paths uploaded to sc.off / sc.px / sc.py
    const TickPlanner& t = P[who[0]];
    hipLaunchKernelGGL(init_path_batch_kernel, dim3((unsigned)who.size()), dim3(kThreads), 0, h->stream, sc.cand, sc.off, sc.px, sc.py,
                       h->cfg.max_vel_x, h->cfg.acc_lim_x, t.start[2], t.goal[2], h->cfg.min_samples, p->allow_init_with_backwards_motion, h->err_flag.p);
    return TEB_AMD_OK;
  }
  int signatures(std::vector<TickPlanner>&, const std::vector<int>& who, const std::vector<int>&) {
    return launch_signatures(h, nullptr, sc.cand, (int)who.size(), who.size() * (size_t)h->M, p->h_signature_prescaler, sc.sig);
  }
};

// A scene set: one planner per scene (planner s = scene s), every step one launch over the scenes through the ex_* scratch
struct FleetRoute {
  teb_amd_handle* h;
  const teb_amd_hcp_params_t* p;
  TickScratch sc;
  int per_round;           // paths per scene and round
  std::vector<int> off;    // staging of plans() and lines(): read by the stream until the synchronisation after the signatures
  std::vector<double> px, py, pyaw;
  // The initialisers read their parameters from the class of the candidate's scene (F.cfgs / F.class_of_scene, the table a fleet
  // launch reads: the map's, or the handle's configuration alone) through the candidate -> scene array F.ex_scene.
  int candidate_scenes(const std::vector<int>& who) {
    HIPCHK(hipMemcpyAsync(h->fleet.ex_scene.p, who.data(), who.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return TEB_AMD_OK;
  }
  int plans(std::vector<TickPlanner>& P, const std::vector<int>& who) {   // addAndInitNewTeb(*initial_plan_, ...) of every scene
    auto& F = h->fleet;
    off.assign(1, 0); px.clear(); py.clear(); pyaw.clear();
    for (int s : who) {
      const TickPlanner& t = P[s];
      px.insert(px.end(), t.plan_x, t.plan_x + t.n_plan); py.insert(py.end(), t.plan_y, t.plan_y + t.n_plan);
      pyaw.insert(pyaw.end(), t.plan_yaw, t.plan_yaw + t.n_plan);
      off.push_back((int)px.size());
    }
    HIPCHK(hipMemcpyAsync(sc.off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(sc.px, px.data(), px.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(sc.py, py.data(), py.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(F.ex_pyaw.p, pyaw.data(), pyaw.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->err_flag.p, 0, sizeof(int), h->stream));
    if (int rc = candidate_scenes(who)) return rc;
    hipLaunchKernelGGL(init_plan_fleet_kernel, dim3((unsigned)who.size()), dim3(kThreads), 0, h->stream, sc.cand, sc.off, sc.px, sc.py,
                       F.ex_pyaw.p, F.ex_scene.p, F.cfgs.p, F.class_of_scene.p, p->global_plan_overwrite_orientation,
                       p->allow_init_with_backwards_motion, h->err_flag.p);
    return TEB_AMD_OK;
  }
  int lines(std::vector<TickPlanner>& P, const std::vector<int>& who) {   // addAndInitNewTeb(start, goal, ...) of every scene at its goal
    auto& F = h->fleet;
    px.assign(6 * who.size(), 0.0);   // (start, goal) of every line
    for (size_t k = 0; k < who.size(); ++k)
      for (int j = 0; j < 3; ++j) { px[6 * k + j] = P[who[k]].start[j]; px[6 * k + 3 + j] = P[who[k]].goal[j]; }
    HIPCHK(hipMemcpyAsync(F.ex_line.p, px.data(), px.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->err_flag.p, 0, sizeof(int), h->stream));
    if (int rc = candidate_scenes(who)) return rc;
    hipLaunchKernelGGL(init_line_fleet_kernel, dim3((unsigned)who.size()), dim3(kThreads), 0, h->stream, sc.cand, F.ex_line.p, F.ex_scene.p, F.cfgs.p,
                       F.class_of_scene.p, 0.0, p->allow_init_with_backwards_motion, h->err_flag.p);
    return TEB_AMD_OK;
  }
  int edges(std::vector<TickPlanner>& P, const std::vector<int>& who) {   // every graph in one launch, one download
    auto& F = h->fleet;
    size_t nv = 0, na = 0, most = 0;
    for (int s : who) { const size_t N = P[s].vx.size(); nv += N; na += N * N; most = std::max(most, N * N); }
    if (F.ex_gvx.n < nv) { F.ex_gvx.free(); F.ex_gvy.free(); HIPCHK(F.ex_gvx.alloc(nv)); HIPCHK(F.ex_gvy.alloc(nv)); }
    if (F.ex_gadj.n < na) { F.ex_gadj.free(); HIPCHK(F.ex_gadj.alloc(na)); }
    std::vector<double> allx, ally, orient(2 * P.size(), 0.0);   // orient: of start and goal, for the path bands of the rounds
    std::vector<GraphFleetRec> recs(who.size());
    size_t vo = 0, ao = 0;
    for (size_t i = 0; i < who.size(); ++i) {
      TickPlanner& t = P[who[i]];
      const size_t N = t.vx.size();
      allx.insert(allx.end(), t.vx.begin(), t.vx.end()); ally.insert(ally.end(), t.vy.begin(), t.vy.end());
      t.ga.N = (int)N; t.ga.gx = F.ex_gvx.p + vo; t.ga.gy = F.ex_gvy.p + vo; t.ga.adj = F.ex_gadj.p + ao;
      recs[i].g = t.ga; recs[i].scene = who[i];
      vo += N; ao += N * N;
    }
    for (size_t s = 0; s < P.size(); ++s) { orient[2 * s] = P[s].start[2]; orient[2 * s + 1] = P[s].goal[2]; }
    HIPCHK(hipMemcpyAsync(F.ex_gvx.p, allx.data(), nv * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(F.ex_gvy.p, ally.data(), nv * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(F.ex_rec.p, recs.data(), recs.size() * sizeof(GraphFleetRec), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(F.ex_orient.p, orient.data(), orient.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    LAUNCH(graph_edges_fleet_kernel, dim3((unsigned)((most + kThreads - 1) / kThreads), (unsigned)who.size()), dim3(kThreads), 0, h->stream, F.scenes.p,
           F.ex_rec.p);
    std::vector<unsigned char> adjm(na);
    HIPCHK(hipMemcpyAsync(adjm.data(), F.ex_gadj.p, na, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    ao = 0;
    for (int s : who) { const size_t NN = P[s].vx.size() * P[s].vx.size(); P[s].mem->g_adj.assign(adjm.begin() + ao, adjm.begin() + ao + NN); ao += NN; }
    return TEB_AMD_OK;
  }
  int paths(std::vector<TickPlanner>&, const std::vector<int>& who) {   // the paths uploaded to sc.off / sc.px / sc.py
    auto& F = h->fleet;
    if (int rc = candidate_scenes(who)) return rc;
    hipLaunchKernelGGL(init_path_fleet_kernel, dim3((unsigned)who.size()), dim3(kThreads), 0, h->stream, sc.cand, sc.off, sc.px, sc.py,
                       F.ex_scene.p, F.ex_orient.p, F.cfgs.p, F.class_of_scene.p, p->allow_init_with_backwards_motion, h->err_flag.p);
    return TEB_AMD_OK;
  }
  int signatures(std::vector<TickPlanner>&, const std::vector<int>& who, const std::vector<int>& soff) {
    auto& F = h->fleet;
    const size_t total = (size_t)soff.back();
    HIPCHK(hipMemcpyAsync(F.ex_scene.p, who.data(), who.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    FleetHsigDev fl;
    fl.scenes = F.scenes.p; fl.scene_of = F.ex_scene.p; fl.off = F.ex_soff.p;
    if (agreed_cfg(h, true).include_dynamic_obstacles && total > 0)
      HIPCHK(hipMemcpyAsync(F.ex_soff.p, soff.data(), soff.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    return launch_signatures(h, &fl, sc.cand, (int)who.size(), total, p->h_signature_prescaler, sc.sig);
  }
};

// plans -> vertices -> edges -> rounds -> at-goal lines for the planners P; their class tables are seeded, their outputs initialised
extern "C++" template <class Route>
int explore_tick(teb_amd_handle* h, const teb_amd_hcp_params_t* p, Route& R, std::vector<TickPlanner>& P, int free_goal_vel, int64_t max_paths) {
  // the candidates of a launch: planner of every candidate, its signature values at sig[soff[k] ..), the accepted ones, the paths of a round
  std::vector<int> who, soff, acc, off;
  std::vector<double> sig, px, py;
  auto classify = [&]() -> int {
    const int count = (int)who.size();
    soff.assign(count + 1, 0);
    for (int k = 0; k < count; ++k) soff[k + 1] = soff[k] + P[who[k]].ct.sig.W;
    const size_t total = (size_t)soff[count];
    sig.assign(std::max<size_t>(total, 1), 0.0);
    HIPCHK(hipGetLastError());   // of the launch that initialised the candidates
    if (int rc = R.signatures(P, who, soff)) return rc;
    if (total > 0) HIPCHK(hipMemcpyAsync(sig.data(), R.sc.sig, total * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    int err = 0;
    HIPCHK(hipMemcpyAsync(&err, h->err_flag.p, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (err) return fail(TEB_AMD_ERR_CAPACITY, "candidate band needs more poses than max_poses");
    return TEB_AMD_OK;
  };
  auto append = [&]() { return append_candidates(h, R.sc, acc, who, P, free_goal_vel); };
  // one candidate for every planner of `who`, a band where its class is new: the initial plan (addAndInitNewTeb(*initial_plan_, ...),
  // hcp.cpp:326-329, 412-440; its class is initial_plan_eq_class_) or the line from start to goal (addAndInitNewTeb(start, goal, ...), :358-384)
  auto one_each = [&](bool plan) -> int {
    if (who.empty()) return TEB_AMD_OK;
    acc.clear();
    int rc = plan ? R.plans(P, who) : R.lines(P, who);
    if (rc || (rc = classify())) return rc;
    for (size_t k = 0; k < who.size(); ++k) {
      TickPlanner& t = P[who[k]];
      const double* v = sig.data() + soff[k];
      if (plan) { t.mem->initial_class.assign(v, v + t.ct.sig.W); t.mem->initial_class_mode = t.ct.sig.mode; }
      if (t.ct.add_if_new(v)) { acc.push_back((int)k); if (plan) t.created = (int)t.bands.size(); }
    }
    return append();
  };
  // ---- the initial plans as first candidates -----------------------------------------------------------------------------------------
  for (size_t i = 0; i < P.size(); ++i) if (P[i].n_plan > 0 && !P[i].full()) who.push_back((int)i);
  if (int rc = one_each(true)) return rc;
  // ---- vertices, on the host planner by planner; the planners that return before their graph -----------------------------------------
  std::vector<int> graphs, at_goal;
  for (size_t i = 0; i < P.size(); ++i) {
    TickPlanner& t = P[i];
    if (t.full()) continue;
    const double dfx = t.goal[0] - t.start[0], dfy = t.goal[1] - t.start[1];
    const double start_goal_dist = std::sqrt(dfx * dfx + dfy * dfy);
    if (start_goal_dist < p->xy_goal_tolerance) {                             // src/graph_search.cpp:104-113, 237-246
      if (t.bands.empty()) at_goal.push_back((int)i);                         // a line band, and only for a planner without any band
      continue;
    }
    graph_vertices(*t.tab, t.start, t.goal, start_goal_dist, t.dist_to_obst, p, t.mem->rnd, t.unit_samples, t.vx, t.vy, t.ga);
    if (t.n_vertices) *t.n_vertices = (int32_t)t.vx.size();
    graphs.push_back((int)i);
  }
  // ---- edges (device), then the graph is what the planner remembers ------------------------------------------------------------------
  if (!graphs.empty()) {
    if (int rc = R.edges(P, graphs)) return rc;
    for (int i : graphs) {
      TickPlanner& t = P[i];
      t.mem->g_vx = t.vx; t.mem->g_vy = t.vy;
      t.paths = PathSource(adjacency_lists(t.mem->g_adj.data(), (int)t.vx.size()), max_paths);
    }
  }
  // ---- rounds: up to per_round paths of every planner with room and paths left; init + signature on the device, then first come first served
  for (;;) {
    off.assign(1, 0); px.clear(); py.clear(); who.clear(); acc.clear();
    for (int i : graphs) {
      TickPlanner& t = P[i];
      if (!t.paths.more || t.full()) continue;
      const int count = take_paths(t.paths, R.per_round, max_paths, h->stride + 1, t.vx, t.vy, px, py, off);
      if (count < 0) return fail(TEB_AMD_ERR_CAPACITY, "a start-goal path has more vertices than a band has poses (max_poses)");
      who.insert(who.end(), (size_t)count, i);
    }
    if (who.empty()) break;
    HIPCHK(hipMemcpyAsync(R.sc.off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(R.sc.px, px.data(), px.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(R.sc.py, py.data(), py.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemsetAsync(h->err_flag.p, 0, sizeof(int), h->stream));
    int rc = R.paths(P, who);
    if (rc || (rc = classify())) return rc;
    for (size_t k = 0; k < who.size();) {
      TickPlanner& t = P[who[k]];
      const int count = (int)(std::find_if(who.begin() + k, who.end(), [&](int w) { return w != who[k]; }) - (who.begin() + k));
      t.paths.examined += accept_in_order(t.ct, sig.data() + soff[k], (int)k, count, t.slots - (int)t.bands.size(), acc);
      k += count;
    }
    if ((rc = append())) return rc;
  }
  for (int i : graphs)
    if (P[i].n_paths) *P[i].n_paths = (int32_t)std::min<int64_t>(P[i].paths.examined, std::numeric_limits<int32_t>::max());
  // ---- the planners at their goal without a band: their line bands ------------------------------------------------------------------
  who = at_goal;
  return one_each(false);
}

// getInitialPlanTEB (:495-536) and updateReferenceTrajectoryViaPoints (:286-315) planner by planner after a tick; one upload of via_en
int finish_tick(teb_amd_handle* h, const teb_amd_hcp_params_t* p, std::vector<TickPlanner>& P) {
  std::vector<std::vector<int>> rule(P.size());
  bool any = false;
  for (size_t i = 0; i < P.size(); ++i) {
    TickPlanner& t = P[i];
    const int n = (int)t.bands.size();
    if (t.initial_plan_teb) *t.initial_plan_teb = initial_plan_band(t.ct, *t.mem, n, t.created);
    if (via_point_rule(t.ct, *t.mem, n, p->viapoints_all_candidates != 0, t.n_plan > 0, t.n_via, t.weight_viapoint, rule[i])) any = true;
  }
  if (!any) return TEB_AMD_OK;
  std::vector<int> ve(h->B, 0);
  if (P.size() > 1) {   // the bands of a planner whose rule does not run keep their flags
    HIPCHK(hipMemcpyAsync(ve.data(), h->bands.via_en.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  for (size_t i = 0; i < P.size(); ++i)
    for (size_t b = 0; b < rule[i].size(); ++b) ve[P[i].bands[b]] = rule[i][b];
  HIPCHK(hipMemcpyAsync(h->bands.via_en.p, ve.data(), h->B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  return synced(h);
}

int copy_graph(const PlannerMemory& m, double* vx, double* vy, unsigned char* adjacency, int32_t capacity_vertices, int32_t* n_vertices) {
  const int N = (int)m.g_vx.size();
  if (n_vertices) *n_vertices = N;
  if (N == 0 || (!vx && !vy && !adjacency)) return TEB_AMD_OK;
  if (capacity_vertices < N) return fail(TEB_AMD_ERR_CAPACITY, "graph has more vertices than capacity_vertices");
  if (vx) std::copy(m.g_vx.begin(), m.g_vx.end(), vx);
  if (vy) std::copy(m.g_vy.begin(), m.g_vy.end(), vy);
  if (adjacency) std::copy(m.g_adj.begin(), m.g_adj.end(), adjacency);
  return TEB_AMD_OK;
}
}  // namespace

int teb_amd_explore_candidates(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const double* start, const double* goal,
                               double dist_to_obst, const double* start_vel, int32_t free_goal_vel, int32_t best,
                               const double* unit_samples, int64_t max_paths, int32_t* n_total, int32_t* n_vertices, int32_t* n_paths,
                               int32_t n_plan, const double* plan_x, const double* plan_y, const double* plan_yaw,
                               int32_t* initial_plan_teb) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_explore_candidates"))) return rc;
  if (!p || !start || !goal) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  if (n_plan > 0 && (!plan_x || !plan_y || !plan_yaw)) return fail(TEB_AMD_ERR_INVALID_ARG, "null initial plan");
  if (initial_plan_teb) *initial_plan_teb = -1;
  if ((rc = ensure_candidate_buffers(h))) return rc;
  const int mode = h->cfg.include_dynamic_obstacles ? 3 : 2, W = mode == 3 ? h->M : 2;
  h->memory.forget_graph();
  if (n_vertices) *n_vertices = 0;
  if (n_paths) *n_paths = 0;
  if (n_total) *n_total = h->B;
  std::vector<TickPlanner> P(1);
  TickPlanner& t = P[0];
  t.tab = &h->hob; t.mem = &h->memory; t.start = start; t.goal = goal; t.start_vel = start_vel;
  t.n_plan = n_plan; t.plan_x = plan_x; t.plan_y = plan_y; t.plan_yaw = plan_yaw; t.unit_samples = unit_samples;
  t.slots = std::min<int>(p->max_number_classes, h->max_tebs); t.n_via = h->nvia;
  t.dist_to_obst = dist_to_obst; t.weight_viapoint = h->cfg.weight_viapoint;
  t.n_vertices = n_vertices; t.n_paths = n_paths; t.initial_plan_teb = initial_plan_teb;
  // equivalence_classes_ of the existing bands
  std::vector<const double*> rows;
  if (h->B > 0) {
    if (!h->sigs.fresh(mode, h->B, p->h_signature_prescaler, (long long)h->B * W) &&   // else: renew just did
        (rc = teb_amd_compute_h_signatures(h, p->h_signature_prescaler, nullptr, nullptr))) return rc;
    rows = h->sigs.rows();
    for (int b = 0; b < h->B; ++b) t.bands.push_back(b);
  }
  t.ct = seed_class_table(SignatureRule{mode, W, p->h_signature_threshold}, p->max_number_plans_in_current_class, rows,
                          best >= 0 && best < h->B ? rows[best] : nullptr, h->memory);
  h->bands_changed();   // the batch is about to change: signatures have to be recomputed before the next filter call
  SingleRoute R{h, p, {batch_of(h), h->cand_map.p, h->cand_off.p, h->cand_px.p, h->cand_py.p, h->cand_sig.p}, kCandChunk};
  h->cand.into(R.sc.cand);   // the scratch strips seen as a batch of kCandChunk bands
  if ((rc = explore_tick(h, p, R, P, free_goal_vel, max_paths))) return rc;
  if (n_total) *n_total = h->B;
  return finish_tick(h, p, P);
}

int teb_amd_get_exploration_graph(teb_amd_handle_t* h, double* vx, double* vy, unsigned char* adjacency, int32_t capacity_vertices,
                                  int32_t* n_vertices) {
  if (int rc = check_handle(h)) return rc;
  return copy_graph(h->memory, vx, vy, adjacency, capacity_vertices, n_vertices);
}

// ---- candidate generation per scene of a fleet batch (teb_amd.h, fleet batches; kernels: the fleet forms of teb_graph.hpp) ----------
namespace {
// teb_amd_explore_candidates_per_scene (dist_to_obst: the one value of the call) and teb_amd_explore_candidates_per_class (null: every
// scene takes min_obstacle_dist of its class). Everything else a scene reads from a configuration is that of its class either way.
int explore_per_scene(teb_amd_handle* h, const char* fn, const teb_amd_hcp_params_t* p, const double* start, const double* goal,
                      const double* dist_to_obst, const double* start_vel, int32_t free_goal_vel, const int32_t* best,
                      const double* unit_samples, int64_t max_paths, int32_t* n_total, int32_t* n_bands, int32_t* n_vertices, int32_t* n_paths,
                      const int32_t* plan_count, const double* plan_x, const double* plan_y, const double* plan_yaw, int32_t* initial_plan_teb) {
  int rc = TEB_AMD_OK;
  auto& F = h->fleet;
  const ClassList cl = fleet_classes(h);
  const int ns = F.n_scenes, B0 = h->B;
  std::vector<int> plan_off(ns + 1, 0);
  for (int s = 0; s < ns; ++s) {
    const int np = plan_count ? plan_count[s] : 0;
    if (np < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "negative plan_count");
    if (np > 0 && (!plan_x || !plan_y || !plan_yaw)) return fail(TEB_AMD_ERR_INVALID_ARG, "null initial plan");
    if (np > h->stride + 1) return fail(TEB_AMD_ERR_CAPACITY, "plan / path longer than max_poses + 1");
    plan_off[s + 1] = plan_off[s] + np;
  }
  BandGroups G;   // the bands of every scene in band order
  if ((rc = scene_groups(h, B0, G)) || (rc = check_best_per_scene(G, best, fn))) return rc;
  std::vector<std::vector<int>>& of = G.of;
  const int slots = p->max_number_classes;   // per scene (the reference handle of the contract has max_tebs >= max_number_classes)
  {
    long long need = 0;
    for (int s = 0; s < ns; ++s) need += std::max<long long>((long long)of[s].size(), slots);
    if (need > h->max_tebs) {
      char buf[200];
      std::snprintf(buf, sizeof buf, "%s: %d scenes may grow to %lld bands, max_tebs is %d", fn, ns, need, h->max_tebs);
      return fail(TEB_AMD_ERR_CAPACITY, buf);
    }
  }
  const int mode = agreed_cfg(h, true).include_dynamic_obstacles ? 3 : 2;
  int widest = 0;
  for (const HostObst& t : F.tabs) widest = std::max(widest, (int)t.rows());
  const int q = h->explore_quota > 0 ? h->explore_quota : kExploreQuota;
  const size_t K = std::max<size_t>(kCandChunk, (size_t)q * ns);
  if ((rc = ensure_fleet_candidate_buffers(h, K, K * (size_t)std::max(widest, 2)))) return rc;
  for (int s = 0; s < ns; ++s) {
    F.memory[s].forget_graph();
    if (n_vertices) n_vertices[s] = 0;
    if (n_paths) n_paths[s] = 0;
    if (n_bands) n_bands[s] = (int)of[s].size();
    if (initial_plan_teb) initial_plan_teb[s] = -1;
  }
  if (n_total) *n_total = B0;
  // equivalence_classes_ of the existing bands, one table per scene
  if (B0 > 0) {
    if (!F.sigs.fresh(mode, B0, p->h_signature_prescaler) &&
        (rc = teb_amd_compute_h_signatures_per_scene(h, p->h_signature_prescaler, nullptr, 0, nullptr, nullptr))) return rc;
  }
  std::vector<TickPlanner> P(ns);
  for (int s = 0; s < ns; ++s) {
    TickPlanner& t = P[s];
    const int np = plan_off[s + 1] - plan_off[s];
    t.tab = &F.tabs[s]; t.mem = &F.memory[s];
    t.start = start + 3 * s; t.goal = goal + 3 * s; t.start_vel = start_vel ? start_vel + 3 * s : nullptr;
    t.n_plan = np;
    if (np > 0) { t.plan_x = plan_x + plan_off[s]; t.plan_y = plan_y + plan_off[s]; t.plan_yaw = plan_yaw + plan_off[s]; }
    t.unit_samples = unit_samples ? unit_samples + (size_t)s * 2 * std::max(p->roadmap_graph_no_samples, 0) : nullptr;
    t.slots = slots; t.n_via = F.via_count[s];
    const SceneTickParams tp = scene_tick_params(cl.cfgs, cl.n, cl.class_of, s);
    t.dist_to_obst = dist_to_obst ? *dist_to_obst : tp.dist_to_obst; t.weight_viapoint = tp.weight_viapoint;
    t.n_vertices = n_vertices ? n_vertices + s : nullptr; t.n_paths = n_paths ? n_paths + s : nullptr;
    t.initial_plan_teb = initial_plan_teb ? initial_plan_teb + s : nullptr;
    std::vector<const double*> rows;
    for (int b : of[s]) rows.push_back(F.sigs.row(b));
    t.ct = seed_class_table(SignatureRule{mode, mode == 3 ? (int)F.tabs[s].rows() : 2, p->h_signature_threshold}, p->max_number_plans_in_current_class,
                            rows, best && best[s] >= 0 ? F.sigs.row(best[s]) : nullptr, F.memory[s]);
    t.bands = std::move(of[s]);
  }
  h->bands_changed();   // the batch is about to change
  FleetRoute R{h, p, {batch_of(h), F.ex_map.p, F.ex_off.p, F.ex_px.p, F.ex_py.p, F.ex_sig.p}, q, {}, {}, {}, {}};
  F.ex.into(R.sc.cand);   // the scratch strips of the scene set seen as a batch of K bands (they may hold more)
  R.sc.cand.B = (int)K;
  rc = explore_tick(h, p, R, P, free_goal_vel, max_paths);
  if (n_total) *n_total = h->B;
  for (int s = 0; s < ns; ++s) if (n_bands) n_bands[s] = (int)P[s].bands.size();
  if (rc) return rc;
  return finish_tick(h, p, P);
}
}  // namespace

int teb_amd_explore_candidates_per_scene(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const double* start, const double* goal,
                                         double dist_to_obst, const double* start_vel, int32_t free_goal_vel, const int32_t* best,
                                         const double* unit_samples, int64_t max_paths, int32_t* n_total, int32_t* n_bands,
                                         int32_t* n_vertices, int32_t* n_paths, const int32_t* plan_count, const double* plan_x,
                                         const double* plan_y, const double* plan_yaw, int32_t* initial_plan_teb) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_explore_candidates_per_scene"))) return rc;
  if (!p || !start || !goal) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  if (h->fleet.classes.size() > 1)   // dist_to_obst is one value per call: the classes' min_obstacle_dist have no place in it (teb_amd_explore_candidates_per_class)
    return fail(TEB_AMD_ERR_UNSUPPORTED, "teb_amd_explore_candidates_per_scene: not available while a class map with more than one class is installed (teb_amd_set_scene_configs)");
  return explore_per_scene(h, "teb_amd_explore_candidates_per_scene", p, start, goal, &dist_to_obst, start_vel, free_goal_vel, best, unit_samples,
                           max_paths, n_total, n_bands, n_vertices, n_paths, plan_count, plan_x, plan_y, plan_yaw, initial_plan_teb);
}

int teb_amd_explore_candidates_per_class(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const double* start, const double* goal,
                                         const double* start_vel, int32_t free_goal_vel, const int32_t* best, const double* unit_samples,
                                         int64_t max_paths, int32_t* n_total, int32_t* n_bands, int32_t* n_vertices, int32_t* n_paths,
                                         const int32_t* plan_count, const double* plan_x, const double* plan_y, const double* plan_yaw,
                                         int32_t* initial_plan_teb) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_explore_candidates_per_class"))) return rc;
  if (!p || !start || !goal) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  return explore_per_scene(h, "teb_amd_explore_candidates_per_class", p, start, goal, nullptr, start_vel, free_goal_vel, best, unit_samples,
                           max_paths, n_total, n_bands, n_vertices, n_paths, plan_count, plan_x, plan_y, plan_yaw, initial_plan_teb);
}

int teb_amd_get_exploration_graph_per_scene(teb_amd_handle_t* h, int32_t scene, double* vx, double* vy, unsigned char* adjacency,
                                            int32_t capacity_vertices, int32_t* n_vertices) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_get_exploration_graph_per_scene"))) return rc;
  if (scene < 0 || scene >= h->fleet.n_scenes) return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_get_exploration_graph_per_scene: scene out of range");
  return copy_graph(h->fleet.memory[scene], vx, vy, adjacency, capacity_vertices, n_vertices);
}

namespace {
// The bands map[0 .. K) (indices into the batch) become bands 0 .. K - 1, with their attributes, their signatures of the single scene
// and their entries of the band -> scene map; B = K afterwards.
int compact_by_map(teb_amd_handle* h, const std::vector<int>& map) {
  const int B = h->B;
  if (!h->tmp.allocated()) {
    if (ensure_candidate_buffers(h) != TEB_AMD_OK || h->tmp.alloc(h->max_tebs, h->stride) != hipSuccess) return fail(TEB_AMD_ERR_HIP, "compaction scratch allocation failed");
  }
  const int K = (int)map.size();
  bool identity = true;
  for (int k = 0; k < K; ++k) if (map[k] != k) identity = false;
  if (!identity && K > 0) {
    BatchDev src = batch_of(h), tmp = src;
    h->tmp.view(tmp);
    std::vector<int> ident(K);
    for (int k = 0; k < K; ++k) ident[k] = k;
    HIPCHK(hipMemcpyAsync(h->cand_map.p, map.data(), K * sizeof(int), hipMemcpyHostToDevice, h->stream));
    LAUNCH(move_bands_kernel, dim3(K), dim3(kThreads), 0, h->stream, src, tmp, h->cand_map.p, 0, 1);
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpyAsync(h->cand_map.p, ident.data(), K * sizeof(int), hipMemcpyHostToDevice, h->stream));
    LAUNCH(move_bands_kernel, dim3(K), dim3(kThreads), 0, h->stream, tmp, src, h->cand_map.p, 0, 1);
    HIPCHK(hipStreamSynchronize(h->stream));
  }
  // the single scene's signatures travel with their bands (same rows, new order); the scene set's are computed again
  if (h->sigs.mode != 0 && h->sigs.B == B) h->sigs.gather(map); else h->sigs.clear();
  h->fleet.sigs.clear();
  if (!h->fleet.band_scene.empty()) {   // the band -> scene map (teb_amd_set_band_scenes) travels with the bands; the freed slots: scene 0
    auto& F = h->fleet;
    std::vector<int> moved(F.band_scene.size(), 0);
    for (int k = 0; k < K; ++k) moved[k] = F.band_scene[map[k]];
    if (moved != F.band_scene) {
      F.band_scene.swap(moved);
      if (F.allocated) {
        HIPCHK(hipMemcpyAsync(F.scene_of.p, F.band_scene.data(), F.band_scene.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
      }
    }
  }
  h->B = K;
  h->bands_changed(-1, false);
  return TEB_AMD_OK;
}

// The erase of the dropped bands of the planners G (compaction_map of teb_hcp_host.hpp): best and new_best [groups] or NULL
int compact_groups(teb_amd_handle* h, const BandGroups& G, const int32_t* keep, const int32_t* best, int32_t* n_kept, int32_t* new_best) {
  std::vector<int> map;
  std::vector<int32_t> nb(G.size());
  compaction_map(G, keep, best, map, nb.data());
  if (int rc = compact_by_map(h, map)) return rc;
  if (new_best) std::copy(nb.begin(), nb.end(), new_best);
  if (n_kept) *n_kept = (int)map.size();
  return TEB_AMD_OK;
}

// detour_stats_kernel over all B bands: st [4 * B], opt [B]
int detour_statistics(teb_amd_handle* h, const teb_amd_hcp_params_t* p, int B, std::vector<double>& st, std::vector<int>& opt) {
  if (int rc = ensure_candidate_buffers(h)) return rc;
  LAUNCH(detour_stats_kernel, dim3(B), dim3(kThreads), 0, h->stream, batch_of(h), p->length_start_orientation_vector, h->cand_sig.p);
  st.assign((size_t)4 * B, 0.0);
  opt.assign(B, 0);
  HIPCHK(hipMemcpyAsync(st.data(), h->cand_sig.p, st.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(opt.data(), h->bands.optimized.p, B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

// deletePlansDetouringBackwards of the planners G, best [groups]: one launch over all bands if any planner is past its early-out
int filter_detours(teb_amd_handle* h, const teb_amd_hcp_params_t* p, const BandGroups& G, const int32_t* best, int32_t* keep) {
  std::vector<int> runs;
  for (int g = 0; g < G.size(); ++g)
    if (detour_rule_runs(G.of[g], best[g], keep)) runs.push_back(g);
  if (runs.empty()) return TEB_AMD_OK;
  std::vector<double> st;
  std::vector<int> opt;
  if (int rc = detour_statistics(h, p, G.B, st, opt)) return rc;
  for (int g : runs) apply_detour_rule(G.of[g], best[g], p, st.data(), opt.data(), keep);
  return TEB_AMD_OK;
}
}  // namespace

int teb_amd_compact_bands(teb_amd_handle_t* h, const int32_t* keep, int32_t best, int32_t* n_kept, int32_t* new_best) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!keep) return fail(TEB_AMD_ERR_INVALID_ARG, "null keep");
  if (new_best) *new_best = -1;
  if (n_kept) *n_kept = 0;
  if (h->B <= 0) return TEB_AMD_OK;
  return compact_groups(h, BandGroups(1, h->B, nullptr), keep, &best, n_kept, new_best);   // (a best that is no band: none, not refused)
}

int teb_amd_compact_bands_per_scene(teb_amd_handle_t* h, const int32_t* keep, const int32_t* best, int32_t* n_kept, int32_t* new_best) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_compact_bands_per_scene"))) return rc;
  if (!keep) return fail(TEB_AMD_ERR_INVALID_ARG, "null keep");
  if (new_best) std::fill(new_best, new_best + h->fleet.n_scenes, -1);
  if (n_kept) *n_kept = 0;
  if (h->B <= 0) return TEB_AMD_OK;
  BandGroups G;
  if ((rc = scene_groups(h, h->B, G)) || (rc = check_best_per_scene(G, best, "teb_amd_compact_bands_per_scene"))) return rc;
  return compact_groups(h, G, keep, best, n_kept, new_best);
}

int teb_amd_filter_detours(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, int32_t best, int32_t* keep) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_filter_detours"))) return rc;
  if (!p || !keep) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  if (h->B <= 0) return TEB_AMD_OK;
  return filter_detours(h, p, BandGroups(1, h->B, nullptr), &best, keep);
}

int teb_amd_filter_detours_per_scene(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const int32_t* best, int32_t* keep) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = require_fleet_mode(h, "teb_amd_filter_detours_per_scene"))) return rc;
  if (!p || !keep) return fail(TEB_AMD_ERR_INVALID_ARG, "null argument");
  if (h->B <= 0) return TEB_AMD_OK;
  BandGroups G;
  if ((rc = scene_groups(h, h->B, G)) || (rc = check_best_per_scene(G, best, "teb_amd_filter_detours_per_scene"))) return rc;
  return best ? filter_detours(h, p, G, best, keep) : (int)TEB_AMD_OK;   // without best bands no planner's rule runs
}

int teb_amd_set_optimized_flags(teb_amd_handle_t* h, const int32_t* flags) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!flags) return fail(TEB_AMD_ERR_INVALID_ARG, "null flags");
  if (h->B <= 0) return TEB_AMD_OK;
  std::vector<int> f(h->B);
  for (int b = 0; b < h->B; ++b) f[b] = flags[b] != 0;
  HIPCHK(hipMemcpyAsync(h->bands.optimized.p, f.data(), h->B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  return synced(h);
}

int teb_amd_get_optimized_flags(teb_amd_handle_t* h, int32_t* flags) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!flags) return fail(TEB_AMD_ERR_INVALID_ARG, "null flags");
  if (h->B <= 0) return TEB_AMD_OK;
  HIPCHK(hipMemcpyAsync(flags, h->bands.optimized.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

int teb_amd_get_band_flags(teb_amd_handle_t* h, int32_t* via_points_enabled, int32_t* has_vel_start, int32_t* has_vel_goal) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (h->B <= 0) return TEB_AMD_OK;
  if (via_points_enabled) HIPCHK(hipMemcpyAsync(via_points_enabled, h->bands.via_en.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (has_vel_start) HIPCHK(hipMemcpyAsync(has_vel_start, h->bands.has_vs.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  if (has_vel_goal) HIPCHK(hipMemcpyAsync(has_vel_goal, h->bands.has_vg.p, h->B * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  return synced(h);
}

int teb_amd_device_state(teb_amd_handle_t* h, void** x, void** y, void** theta, void** dt, void** n, int32_t* stride) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (x) *x = h->bands.strips.x.p; if (y) *y = h->bands.strips.y.p; if (theta) *theta = h->bands.strips.th.p; if (dt) *dt = h->bands.strips.dt.p; if (n) *n = h->bands.strips.n.p;
  if (stride) *stride = h->stride;
  h->bands_changed();   // the caller may write pose counts through `n`: the host's upper bound is void from here on (the kernel guards
                        // itself against counts beyond its LDS strips as well)
  return TEB_AMD_OK;
}

int teb_amd_snapshot_state(teb_amd_handle_t* h) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = copy_strips(h, h->snapshot(), h->live(), h->max_tebs))) return rc;
  h->snap_nmax = h->nmax_known;
  h->snap_B = h->B;
  return TEB_AMD_OK;
}

int teb_amd_restore_state(teb_amd_handle_t* h) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = copy_strips(h, h->live(), h->snapshot(), h->max_tebs))) return rc;
  // snap_nmax bounded the first snap_B bands only; the copy brings back the counts of ALL max_tebs slots, so with another batch size the
  // bound says nothing about the bands beyond the old B
  h->bands_changed(h->B == h->snap_B ? h->snap_nmax : -1);
  return TEB_AMD_OK;
}

int teb_amd_last_launch_info(teb_amd_handle_t* h, int32_t* distance_helpers_per_band, int32_t* solver_helpers_per_band, int32_t* repeated_single_cu) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (distance_helpers_per_band) *distance_helpers_per_band = h->mcu_last_helpers;
  if (solver_helpers_per_band) *solver_helpers_per_band = h->mcu_last_solvers;
  if (repeated_single_cu) *repeated_single_cu = h->mcu_last_repeated;
  return TEB_AMD_OK;
}

int teb_amd_multi_cu_backoff(teb_amd_handle_t* h, int32_t* launches_paused, int32_t* pause_length) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (launches_paused) *launches_paused = h->mcu_backoff.left;
  if (pause_length) *pause_length = h->mcu_backoff.len;
  return TEB_AMD_OK;
}

int teb_amd_last_kernel_ms(teb_amd_handle_t* h, float* ms) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!ms || !h->timed) return fail(TEB_AMD_ERR_INVALID_ARG, "no kernel has been launched yet");
  HIPCHK(hipEventSynchronize(h->ev1.e));
  HIPCHK(hipEventElapsedTime(ms, h->ev0.e, h->ev1.e));
  return TEB_AMD_OK;
}

int teb_amd_capacity(teb_amd_handle_t* h, int32_t* lds_bytes, int32_t* max_poses_supported) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (lds_bytes) *lds_bytes = (int32_t)h->layout.plan.total_bytes;
  if (max_poses_supported) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, h->device));
    int S = kThreads * kPoseIterBandHbm;
    while (S > 2 && lds_bytes_for(S, SOLVER_BANDG, h->lds_limit) > h->lds_limit) --S;   // band in HBM: four poses per lane, as many as its LDS strips hold
    *max_poses_supported = S;
  }
  return TEB_AMD_OK;
}

// ---- test hooks (include/teb_amd_debug.h) -------------------------------------------------------------------
int teb_amd_debug_linearize(teb_amd_handle_t* h, int32_t b, double weight_multiplier, double* H_dense, double* bvec,
                            double* chi2, int32_t* assoc_pose, int32_t* assoc_obst, int32_t assoc_cap, int32_t* assoc_count) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_debug_linearize"))) return rc;
  if (b < 0 || b >= h->B) return fail(TEB_AMD_ERR_INVALID_ARG, "TEB index out of range");
  // run the kernel in debug mode on TEB b only: temporarily view the batch as starting at b
  OptArgs a;
  std::memset(&a, 0, sizeof a);
  a.inner = 1; a.outer = 1; a.no_near_cache = h->opt.no_near_cache != 0; a.debug_linearize = 1; a.debug_weight_multiplier = weight_multiplier; a.band_ldlt = h->layout.solver == SOLVER_BANDG ? 0 : h->band_ldlt; a.Hband = h->Hband.p; a.hband_stride = h->hband_stride;
  a.dbg_H = h->dbg_H.p; a.dbg_b = h->dbg_b.p; a.dbg_chi2 = h->dbg_chi2.p;
  SceneDev sc = scene_of(h);
  BatchDev bt = batch_of(h);
  const size_t so = (size_t)b * h->stride;
  bt.B = 1;
  bt.n += b; bt.x += so; bt.y += so; bt.th += so; bt.dt += so;
  bt.has_vs += b; bt.vs += 3 * b; bt.has_vg += b; bt.vg += 3 * b; bt.rotdir += b; bt.via_en += b;
  bt.status += b; bt.iters += b; bt.last_iters += b; bt.trials += b; bt.chi2 += b; bt.cost += b; bt.lambda += b;
  bt.assoc_cnt += so; bt.assoc += (size_t)b * bt.assoc_cap * h->stride; bt.assoc_overflow += b;
  bt.via_pose += (size_t)b * bt.via_cap; bt.Hbackup += (size_t)b * h->hmat_stride;
  // results of TEB b must not be clobbered by the debug run: save and restore them
  int sv_i[3]; double sv_d[3];
  HIPCHK(hipMemcpy(&sv_i[0], h->bands.status.p + b, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sv_i[1], h->bands.iters.p + b, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sv_i[2], h->bands.trials.p + b, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sv_d[0], h->bands.chi2.p + b, sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sv_d[1], h->bands.cost.p + b, sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&sv_d[2], h->bands.lambda.p + b, sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(launch_opt(h, 1, sc, bt, a, h->layout.solver, h->layout.plan));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(h->bands.status.p + b, &sv_i[0], sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->bands.iters.p + b, &sv_i[1], sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->bands.trials.p + b, &sv_i[2], sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->bands.chi2.p + b, &sv_d[0], sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->bands.cost.p + b, &sv_d[1], sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(h->bands.lambda.p + b, &sv_d[2], sizeof(double), hipMemcpyHostToDevice));
  int n = 0;
  HIPCHK(hipMemcpy(&n, h->bands.strips.n.p + b, sizeof(int), hipMemcpyDeviceToHost));
  const int Nt = 4 * n;
  std::vector<double> Hb((size_t)Nt * kBand), bv(Nt);
  HIPCHK(hipMemcpy(Hb.data(), h->dbg_H.p, Hb.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(bv.data(), h->dbg_b.p, bv.size() * sizeof(double), hipMemcpyDeviceToHost));
  if (chi2) HIPCHK(hipMemcpy(chi2, h->dbg_chi2.p, 4 * sizeof(double), hipMemcpyDeviceToHost));
  if (H_dense) {
    std::fill(H_dense, H_dense + (size_t)Nt * Nt, 0.0);
    for (int r = 0; r < Nt; ++r) {
      bool fr = (r < 3) || (r >= 4 * (n - 1));
      for (int d = 0; d < kBand && d <= r; ++d) {
        double v = fr ? 0.0 : Hb[(size_t)r * kBand + d];   // identity rows of fixed variables are exported as zeros
        H_dense[(size_t)r * Nt + (r - d)] = v;
        H_dense[(size_t)(r - d) * Nt + r] = v;
      }
    }
  }
  if (bvec) for (int r = 0; r < Nt; ++r) bvec[r] = bv[r];
  if (assoc_count) {
    std::vector<int> cnt(n), lst((size_t)bt.assoc_cap * h->stride);
    HIPCHK(hipMemcpy(cnt.data(), h->assoc_cnt.p + so, n * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lst.data(), h->assoc.p + (size_t)b * bt.assoc_cap * h->stride, lst.size() * sizeof(int), hipMemcpyDeviceToHost));
    int k = 0;
    for (int i = 1; i < n - 1; ++i)
      for (int q = 0; q < cnt[i]; ++q) {
        const int ent = lst[(size_t)q * h->stride + i];
        for (int rep = (ent & kAssocTriple) ? 3 : 1; rep > 0; --rep) {
          if (k < assoc_cap) { if (assoc_pose) assoc_pose[k] = i; if (assoc_obst) assoc_obst[k] = h->host_static[ent & kAssocMask]; }
          ++k;
        }
      }
    *assoc_count = k;
  }
  return TEB_AMD_OK;
}

int teb_amd_debug_distance(teb_amd_handle_t* h, int32_t nq, const int32_t* obst_index, const double* x, const double* y,
                           const double* theta, const int32_t* spatio_temporal, const double* t, double* dist, double* grad) {
  int rc = check_handle(h);
  if (rc) return rc;
  if ((rc = refuse_in_fleet_mode(h, "teb_amd_debug_distance"))) return rc;
  if (nq <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "nq <= 0");
  for (int q = 0; q < nq; ++q) if (obst_index[q] < 0 || obst_index[q] >= h->M) return fail(TEB_AMD_ERR_INVALID_ARG, "obstacle index out of range");
  DevBuf<int> d_oi, d_st; DevBuf<double> d_x, d_y, d_th, d_t, d_dist, d_grad;
  HIPCHK(d_oi.alloc(nq)); HIPCHK(d_st.alloc(nq)); HIPCHK(d_x.alloc(nq)); HIPCHK(d_y.alloc(nq)); HIPCHK(d_th.alloc(nq));
  HIPCHK(d_t.alloc(nq)); HIPCHK(d_dist.alloc(nq)); HIPCHK(d_grad.alloc(3 * (size_t)nq));
  HIPCHK(hipMemcpy(d_oi.p, obst_index, nq * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_st.p, spatio_temporal, nq * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_x.p, x, nq * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_y.p, y, nq * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_th.p, theta, nq * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d_t.p, t, nq * sizeof(double), hipMemcpyHostToDevice));
  SceneDev sc = scene_of(h);
  LAUNCH(distance_kernel, dim3((nq + 255) / 256), dim3(256), 0, h->stream, h->cfg, sc, nq, d_oi.p, d_x.p, d_y.p, d_th.p, d_st.p, d_t.p, d_dist.p, d_grad.p);
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(dist, d_dist.p, nq * sizeof(double), hipMemcpyDeviceToHost));
  if (grad) HIPCHK(hipMemcpy(grad, d_grad.p, 3 * (size_t)nq * sizeof(double), hipMemcpyDeviceToHost));
  return TEB_AMD_OK;
}

int teb_amd_debug_profile(teb_amd_handle_t* h, double* cycles8) {
  int rc = check_handle(h);
  if (rc) return rc;
#ifdef TEB_PROFILE
  HIPCHK(hipStreamSynchronize(h->stream));
  HIPCHK(hipMemcpy(cycles8, h->dbg_H.p, 8 * sizeof(double), hipMemcpyDeviceToHost));
  long long crp[8], crw[32];
  HIPCHK(hipMemcpyFromSymbol(crp, HIP_SYMBOL(tebamd::g_cr_prof), sizeof crp));
  HIPCHK(hipMemcpyFromSymbol(crw, HIP_SYMBOL(tebamd::g_crw_prof), sizeof crw));
  for (int w = 0; w < 4; ++w)
    fprintf(stderr, "[cr_forward rounds of %2d-lane groups, workgroup 0 thread 0, cumulative: load+factor | loads+solve3 | Schur products | writes 1 | barrier 1 | writes 2 + barrier 2 | rounds] %lld %lld %lld %lld %lld %lld | %lld\n",
            8 << w, crw[w * 8 + 0], crw[w * 8 + 1], crw[w * 8 + 2], crw[w * 8 + 3], crw[w * 8 + 4], crw[w * 8 + 5], crw[w * 8 + 6]);
  fprintf(stderr, "[cr_solve cycles, workgroup 0, cumulative; hybrid solve: init compact | level 0 | compact forward | top + backward | odd rows] %lld %lld %lld %lld %lld %lld\n",
          crp[0], crp[1], crp[2], crp[3], crp[4], crp[5]);
  unsigned long long ast[4];
  HIPCHK(hipMemcpyFromSymbol(ast, HIP_SYMBOL(tebamd::g_assoc_stats), sizeof ast));
  fprintf(stderr, "[association of generic shapes, all workgroups, cumulative] %llu candidates after the far-field cull, %llu exact distances\n", ast[0], ast[1]);
  unsigned long long ars[4];
  HIPCHK(hipMemcpyFromSymbol(ars, HIP_SYMBOL(tebamd::g_ar_steps), sizeof ars));
  fprintf(stderr, "[autoResize rule machine, workgroup 0, cumulative] %llu calls, %llu steps, %llu cycles\n", ars[2], ars[1], ars[3]);
  unsigned long long nq[2];
  HIPCHK(hipMemcpyFromSymbol(&nq[0], HIP_SYMBOL(tebamd::g_near_recomputed), sizeof nq[0]));
  HIPCHK(hipMemcpyFromSymbol(&nq[1], HIP_SYMBOL(tebamd::g_near_queries), sizeof nq[1]));
  fprintf(stderr, "[near masks of the dynamic-obstacle edges, all workgroups, cumulative] recomputed by %llu of %llu lane passes\n", nq[0], nq[1]);
  long long lnp[16];
  HIPCHK(hipMemcpyFromSymbol(lnp, HIP_SYMBOL(tebamd::g_lin_prof), sizeof lnp));
  fprintf(stderr, "[linearize cycles, thread 0 of workgroup 0, cumulative] zero H, b %lld | trig + barrier %lld | near masks %lld | edges %lld | slice reduction %lld | scatter (3 phases) %lld | tail + chi2 sum %lld\n",
          lnp[0], lnp[1], lnp[2], lnp[3], lnp[4], lnp[5], lnp[6]);
  fprintf(stderr, "[graph side data cycles, thread 0 of workgroup 0, cumulative] trig %lld | association %lld | time stamps (one lane) %lld | via-points + barrier %lld\n",
          lnp[8], lnp[9], lnp[10], lnp[11]);
  long long evp[8];
  HIPCHK(hipMemcpyFromSymbol(evp, HIP_SYMBOL(tebamd::g_ev_prof), sizeof evp));
  fprintf(stderr, "[eval_index cycles, thread 0 of workgroup 0, cumulative] evaluate: static %lld dynamic %lld chain %lld | linearise: static %lld dynamic %lld chain %lld\n",
          evp[0], evp[1], evp[2], evp[3], evp[4], evp[5]);
  return TEB_AMD_OK;
#else
  (void)cycles8;
  return fail(TEB_AMD_ERR_UNSUPPORTED, "library built without -DTEB_PROFILE");
#endif
}

int teb_amd_debug_profile_bands(teb_amd_handle_t* h, double* cycles_per_band) {
  int rc = check_handle(h);
  if (rc) return rc;
#ifdef TEB_PROFILE
  HIPCHK(hipStreamSynchronize(h->stream));
  if ((size_t)16 + h->B > h->dbg_H.n) return fail(TEB_AMD_ERR_CAPACITY, "debug buffer too small");
  HIPCHK(hipMemcpy(cycles_per_band, h->dbg_H.p + 16, h->B * sizeof(double), hipMemcpyDeviceToHost));
  return TEB_AMD_OK;
#else
  (void)cycles_per_band;
  return fail(TEB_AMD_ERR_UNSUPPORTED, "library built without -DTEB_PROFILE");
#endif
}

// debug: checks the operand maps of v_mfma_f64_16x16x4_f64 that cr_forward_mfma relies on (C = A B, A 16x8 row-major, B 8x16, C 16x16)
// and times reps x 4 independent issues on one wave. Builds without -DTEB_AMD_MFMA_SCHUR return TEB_AMD_ERR_UNSUPPORTED.
int teb_amd_debug_mfma_selftest(teb_amd_handle_t* h, const double* A, const double* B, double* C, int32_t reps, double* cycles_per_mfma) {
  int rc = check_handle(h);
  if (rc) return rc;
#ifdef TEB_AMD_MFMA_SCHUR
  if (!A || !B || !C) return fail(TEB_AMD_ERR_INVALID_ARG, "null matrices");
  double *dA = nullptr, *dB = nullptr, *dC = nullptr; long long* dT = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dA), 128 * sizeof(double))); HIPCHK(hipMalloc(reinterpret_cast<void**>(&dB), 128 * sizeof(double)));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&dC), 256 * sizeof(double))); HIPCHK(hipMalloc(reinterpret_cast<void**>(&dT), 2 * sizeof(long long)));
  HIPCHK(hipMemcpyAsync(dA, A, 128 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCHK(hipMemcpyAsync(dB, B, 128 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  LAUNCH(mfma_selftest_kernel, dim3(1), dim3(64), 0, h->stream, dA, dB, dC, reps, dT);
  long long t[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(C, dC, 256 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipMemcpyAsync(t, dT, sizeof(t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  if (cycles_per_mfma) *cycles_per_mfma = reps > 0 ? (double)t[0] / (4.0 * reps) : 0.0;
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC); (void)hipFree(dT);
  return TEB_AMD_OK;
#else
  (void)A; (void)B; (void)C; (void)reps; (void)cycles_per_mfma;
  return fail(TEB_AMD_ERR_UNSUPPORTED, "this build has no MFMA Schur update (-DTEB_AMD_MFMA_SCHUR)");
#endif
}

int teb_amd_debug_stream(teb_amd_handle_t* h, int64_t n_doubles, int32_t repeats) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (n_doubles <= 0 || repeats <= 0) return fail(TEB_AMD_ERR_INVALID_ARG, "bad stream size");
  DevBuf<double> a, b;
  HIPCHK(a.alloc((size_t)n_doubles)); HIPCHK(b.alloc((size_t)n_doubles));
  HIPCHK(hipMemsetAsync(a.p, 0, sizeof(double) * (size_t)n_doubles, h->stream));
  for (int r = 0; r < repeats; ++r) {
    LAUNCH(stream_kernel, dim3(2048), dim3(256), 0, h->stream, a.p, b.p, (size_t)n_doubles);
  }
  HIPCHK(hipStreamSynchronize(h->stream));
  return TEB_AMD_OK;
}

// test hook: overwrites the resident pose count of band b behind the host's back (no range check, the host's cached upper bound of the
// counts is NOT invalidated) - what a careless writer through teb_amd_device_state's `n` pointer could do. The kernel has to survive it.
int teb_amd_debug_poke_pose_count(teb_amd_handle_t* h, int32_t b, int32_t n) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (b < 0 || b >= h->max_tebs) return fail(TEB_AMD_ERR_INVALID_ARG, "band index out of range");
  HIPCHK(hipMemcpyAsync(h->bands.strips.n.p + b, &n, sizeof(int), hipMemcpyHostToDevice, h->stream));
  return synced(h);
}

// diagnostic of the multi-CU mode: from now on every multi-CU launch leaves host-visible breadcrumbs, and one that is still running after
// `milliseconds` prints them and ENDS THE PROCESS (exit code 3). Development tool; 0 switches the watchdog off again.
int teb_amd_debug_mcu_watchdog(teb_amd_handle_t* h, int32_t milliseconds) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (milliseconds > 0 && !h->mcu_trace.p) HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&h->mcu_trace.p), 1024 * sizeof(unsigned), hipHostMallocMapped));
  h->mcu_watchdog_ms = milliseconds;
  return TEB_AMD_OK;
}

// diagnostic of the multi-CU mode: 1 = the association stays with the band's own workgroup, 2 = the distances do (bisecting a difference)
int teb_amd_last_shader_clock_mhz(teb_amd_handle_t* h, double* mhz) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!mhz || !h->timed) return fail(TEB_AMD_ERR_INVALID_ARG, "no kernel has been launched yet");
  long long c[4];
  HIPCHK(hipMemcpyAsync(c, h->clk.p, sizeof(c), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(hipStreamSynchronize(h->stream));
  const double ticks = (double)(c[3] - c[1]);   // 100 MHz real-time counter
  *mhz = ticks > 0 ? (double)(c[2] - c[0]) / ticks * 100.0 : 0.0;
  return TEB_AMD_OK;
}

int teb_amd_debug_rtc_compile(uint64_t flag_values, int32_t solver, int32_t jacobian_mode, int32_t scene_kind, int64_t* code_bytes) {
  if (solver < 0 || solver > 2 || jacobian_mode < 0 || jacobian_mode > 1 || scene_kind < SCENE_POINTS_CUSTOM || scene_kind > SCENE_GENERIC_SMALL_CUSTOM)
    return fail(TEB_AMD_ERR_INVALID_ARG, "teb_amd_debug_rtc_compile: layout 0 .. 2, Jacobian mode 0 / 1, scene kind 12 .. 15");
  RtcKey key;
  key.flags = flag_values; key.solver = solver; key.jmode = jacobian_mode; key.scene = scene_kind;
  std::string why;
  std::shared_ptr<RtcKernel> rk = rtc_request(key, true, &why);
  if (!rk) return fail(TEB_AMD_ERR_UNSUPPORTED, "run-time compilation unavailable: " + why);
  if (rk->state.load() != RtcKernel::READY) return fail(TEB_AMD_ERR_HIP, rk->log.substr(0, 1500));
  if (code_bytes) *code_bytes = (int64_t)rk->code.size();
  return TEB_AMD_OK;
}

#ifndef TEB_AMD_BUILD_SOURCE_HASH
#define TEB_AMD_BUILD_SOURCE_HASH ""   // (a build that did not go through build.py)
#endif
#ifndef TEB_AMD_BUILD_KERNEL_HASH
#define TEB_AMD_BUILD_KERNEL_HASH ""
#endif
int teb_amd_debug_build_info(char* kernel_hash, int32_t kernel_hash_capacity, char* source_hash, int32_t source_hash_capacity, char* variant_defines,
                             int32_t defines_capacity, int32_t* threads_per_workgroup) {
  if (kernel_hash && kernel_hash_capacity > 0) std::snprintf(kernel_hash, (size_t)kernel_hash_capacity, "%s", TEB_AMD_BUILD_KERNEL_HASH);
  if (source_hash && source_hash_capacity > 0) std::snprintf(source_hash, (size_t)source_hash_capacity, "%s", TEB_AMD_BUILD_SOURCE_HASH);
  if (variant_defines && defines_capacity > 0) std::snprintf(variant_defines, (size_t)defines_capacity, "%s", TEB_AMD_VARIANT_DEFINES);
  if (threads_per_workgroup) *threads_per_workgroup = kThreads;
  return TEB_AMD_OK;
}

int teb_amd_debug_rtc_join(void) {   // waits for the background compilations of this process (teb_amd_options_t::compile_for_config = 1) to finish
  rtc_cache().join_workers();
  return TEB_AMD_OK;
}

int teb_amd_debug_rtc_cache(int32_t* embedded, int32_t* disk_hits, int32_t* disk_writes, char* cache_dir, int32_t capacity) {
  RtcCache& c = rtc_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  if (embedded) *embedded = c.embedded ? 1 : 0;
  if (disk_hits) *disk_hits = c.disk_hits.load();
  if (disk_writes) *disk_writes = c.disk_writes.load();
  if (cache_dir && capacity > 0) std::snprintf(cache_dir, (size_t)capacity, "%s", c.disk_dir.c_str());
  return TEB_AMD_OK;
}

int teb_amd_debug_rtc_stats(int32_t* ready, int32_t* compiling, int32_t* failed, double* last_compile_seconds, char* last_error, int32_t capacity) {
  RtcCache& c = rtc_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  int r = 0, w = 0, f = 0;
  double secs = 0;
  std::string err;
  for (auto& kv : c.kernels) {
    const int st = kv.second->state.load();
    if (st == RtcKernel::READY) { ++r; secs = kv.second->compile_seconds; }
    else if (st == RtcKernel::COMPILING) ++w;
    else { ++f; err = kv.second->log; }
  }
  if (ready) *ready = r;
  if (compiling) *compiling = w;
  if (failed) *failed = f;
  if (last_compile_seconds) *last_compile_seconds = secs;
  if (last_error && capacity > 0) { std::snprintf(last_error, (size_t)capacity, "%s", err.c_str()); }
  return TEB_AMD_OK;
}

int teb_amd_debug_last_instantiation(teb_amd_handle_t* h, int32_t* solver, int32_t* jacobian_mode, int32_t* scene_kind) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (solver) *solver = h->last_inst[0];
  if (jacobian_mode) *jacobian_mode = h->last_inst[1];
  if (scene_kind) *scene_kind = h->last_inst[2];
  return TEB_AMD_OK;
}

int teb_amd_debug_last_config_profile(teb_amd_handle_t* h, int32_t* defaults_profile) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (!defaults_profile) return fail(TEB_AMD_ERR_INVALID_ARG, "null output");
  *defaults_profile = h->last_defaults_profile;
  return TEB_AMD_OK;
}

int teb_amd_debug_mcu_flags(teb_amd_handle_t* h, int32_t flags) {
  int rc = check_handle(h);
  if (rc) return rc;
  h->mcu_debug_flags = flags;
  return TEB_AMD_OK;
}


int teb_amd_debug_set_explore_quota(teb_amd_handle_t* h, int32_t quota) {
  int rc = check_handle(h);
  if (rc) return rc;
  if (quota < 0) return fail(TEB_AMD_ERR_INVALID_ARG, "negative quota");
  h->explore_quota = quota;
  return TEB_AMD_OK;
}

int teb_amd_debug_assoc_overflow(teb_amd_handle_t* h, int32_t* flags) {
  int rc = check_handle(h);
  if (rc) return rc;
  HIPCHK(hipMemcpy(flags, h->assoc_ovf.p, h->B * sizeof(int), hipMemcpyDeviceToHost));
  return TEB_AMD_OK;
}

}  // extern "C"
