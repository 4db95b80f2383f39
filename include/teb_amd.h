/*
 * teb_amd.h — C-ABI of the MI355X-native TEB optimiser (libteb_amd.so).
 *
 * This is the drop-in boundary for ONE hot path of rst-tu-dortmund/teb_local_planner:
 *
 *   bool TebOptimalPlanner::optimizeTEB(int iterations_innerloop, int iterations_outerloop,
 *                                       bool compute_cost_afterwards, double obst_cost_scale,
 *                                       double viapoint_cost_scale, bool alternative_time_cost)
 *        reference: include/teb_local_planner/optimal_planner.h:231-232, src/optimal_planner.cpp:182-231
 *   void HomotopyClassPlanner::optimizeAllTEBs(int iter_innerloop, int iter_outerloop)
 *        reference: src/homotopy_class_planner.cpp:466-493
 *   TebOptimalPlannerPtr HomotopyClassPlanner::selectBestTeb()
 *        reference: src/homotopy_class_planner.cpp:564-667
 *
 * Everything is plain C: POD structs, caller-owned fp64 / int32 buffers, an opaque handle, int status
 * codes. No torch / HIP types appear in any signature (streams and device pointers are void*).
 * All arithmetic is fp64 like the reference (Eigen double).
 *
 * The same POD types are consumed by the CPU oracle (oracle/teb_oracle.h, teb_oracle_* symbols); the
 * oracle is test infrastructure and is never linked into libteb_amd.so.
 */
#ifndef TEB_AMD_H_
#define TEB_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TEB_AMD_ABI_VERSION 3
/* Largest pose capacity a handle can be created with on MI355X (band in HBM, four poses per lane; what 160 KB of LDS hold beside the
 * state strips: 951, rounded down to a multiple of 8). trajectory.max_samples (teb_config.h:78) is a parameter of the reference, 500 only
 * by default: bindings size a handle with min(max_samples + 1, TEB_AMD_MAX_POSES). teb_amd_capacity reports the device's own figure. */
#define TEB_AMD_MAX_POSES 944

/* ---- status codes (library calls) ------------------------------------------------------------- */
enum {
  TEB_AMD_OK = 0,
  TEB_AMD_ERR_INVALID_ARG = 1,   /* NULL pointer, negative size, n > max_poses, ...                */
  TEB_AMD_ERR_NO_DEVICE = 2,     /* no HIP device / wrong architecture (no CPU fallback exists)    */
  TEB_AMD_ERR_HIP = 3,           /* a HIP runtime call failed; see teb_amd_last_error()            */
  TEB_AMD_ERR_CAPACITY = 4,      /* max_poses does not fit the per-workgroup LDS budget etc.       */
  TEB_AMD_ERR_UNSUPPORTED = 5    /* feature combination not implemented by this build              */
};

/* ---- per-TEB result status (mirrors the bool returned by optimizeTEB) --------------------------- */
enum {
  TEB_AMD_TEB_OK = 0,            /* optimizeTEB would have returned true                            */
  TEB_AMD_TEB_FAILED = 1,        /* optimizeTEB would have returned false (guards of               */
                                 /*   src/optimal_planner.cpp:185-186, 370-382, 393-397)            */
  TEB_AMD_TEB_NONFINITE = 2      /* a non-finite residual / state was produced (the reference only  */
                                 /*   ROS_ASSERTs on this, e.g. g2o_types/edge_velocity.h:116)      */
};

/* ---- robot footprint models: include/teb_local_planner/robot_footprint_model.h:58-770 ----------- */
enum {
  TEB_AMD_FOOTPRINT_POINT = 0,       /* PointRobotFootprint      :104-176 */
  TEB_AMD_FOOTPRINT_CIRCULAR = 1,    /* CircularRobotFootprint   :229-300 */
  TEB_AMD_FOOTPRINT_TWO_CIRCLES = 2, /* TwoCirclesRobotFootprint :307-430 */
  TEB_AMD_FOOTPRINT_LINE = 3,        /* LineRobotFootprint       :439-635 */
  TEB_AMD_FOOTPRINT_POLYGON = 4      /* PolygonRobotFootprint    :644-770 */
};
#define TEB_AMD_MAX_FOOTPRINT_VERTICES 64   /* (16 until ABI 2; the reference's PolygonRobotFootprint has no limit, robot_footprint_model.h:664-683) */

/* ---- obstacle types: include/teb_local_planner/obstacles.h:67-1111 ------------------------------ */
enum {
  TEB_AMD_OBST_POINT = 0,    /* PointObstacle    (ax,ay)                          */
  TEB_AMD_OBST_CIRCULAR = 1, /* CircularObstacle (ax,ay), radius                  */
  TEB_AMD_OBST_LINE = 2,     /* LineObstacle     (ax,ay)-(bx,by)                  */
  TEB_AMD_OBST_PILL = 3,     /* PillObstacle     (ax,ay)-(bx,by), radius          */
  TEB_AMD_OBST_POLYGON = 4   /* PolygonObstacle  vertices [vert_offset[i], vert_offset[i+1]) */
};

/* ---- RotType: include/teb_local_planner/misc.h:53  (enum class RotType { left, none, right }) --- */
enum { TEB_AMD_ROT_LEFT = 0, TEB_AMD_ROT_NONE = 1, TEB_AMD_ROT_RIGHT = 2 };

/* ---- Jacobian modes (extension; the reference has only the g2o behaviour) ------------------------ */
enum {
  TEB_AMD_JACOBIAN_ANALYTIC = 0,    /* closed-form Jacobians, one-sided conventions of penalties.h:127-187 */
  TEB_AMD_JACOBIAN_G2O_NUMERIC = 1  /* g2o central differences, delta = 1e-9 (Base*Edge::linearizeOplus);  */
                                    /*   EdgeKinematicsDiffDrive / EdgeTimeOptimal stay analytic like the   */
                                    /*   reference (edge_kinematics.h:107-151, edge_time_optimal.h:98-107)  */
};

/*
 * Kernel-relevant subset of TebConfig (include/teb_local_planner/teb_config.h:62-230), same field
 * names, same defaults (teb_config.h:245-390) via teb_amd_config_default(). bools are int32.
 */
typedef struct teb_amd_config {
  /* trajectory */
  int32_t teb_autosize;            /* declared double in the reference, used as bool (teb_config.h:74) */
  double  dt_ref;
  double  dt_hysteresis;
  int32_t min_samples;
  int32_t max_samples;
  int32_t exact_arc_length;
  int32_t via_points_ordered;
  /* robot */
  double  max_vel_x;
  double  max_vel_x_backwards;
  double  max_vel_y;
  double  max_vel_trans;
  double  max_vel_theta;
  double  acc_lim_x;
  double  acc_lim_y;
  double  acc_lim_theta;
  double  min_turning_radius;
  /* obstacles */
  double  min_obstacle_dist;
  double  inflation_dist;
  double  dynamic_obstacle_inflation_dist;
  int32_t include_dynamic_obstacles;
  int32_t obstacle_poses_affected;
  int32_t legacy_obstacle_association;
  double  obstacle_association_force_inclusion_factor;
  double  obstacle_association_cutoff_factor;
  double  obstacle_proximity_ratio_max_vel;
  double  obstacle_proximity_lower_bound;
  double  obstacle_proximity_upper_bound;
  /* optim */
  int32_t no_inner_iterations;
  int32_t no_outer_iterations;
  int32_t optimization_activate;
  double  penalty_epsilon;
  double  weight_max_vel_x;
  double  weight_max_vel_y;
  double  weight_max_vel_theta;
  double  weight_acc_lim_x;
  double  weight_acc_lim_y;
  double  weight_acc_lim_theta;
  double  weight_kinematics_nh;
  double  weight_kinematics_forward_drive;
  double  weight_kinematics_turning_radius;
  double  weight_optimaltime;
  double  weight_shortest_path;
  double  weight_obstacle;
  double  weight_inflation;
  double  weight_dynamic_obstacle;
  double  weight_dynamic_obstacle_inflation;
  double  weight_velocity_obstacle_ratio;
  double  weight_viapoint;
  double  weight_prefer_rotdir;
  double  weight_adapt_factor;
  double  obstacle_cost_exponent;
  /* hcp (selection) */
  double  selection_cost_hysteresis;
  double  selection_prefer_initial_plan;
  double  selection_obst_cost_scale;
  double  selection_viapoint_cost_scale;
  int32_t selection_alternative_time_cost;
  /* recovery */
  int32_t divergence_detection_enable;           /* no constructor default in the reference; 0 here */
  double  divergence_detection_max_chi_squared;  /* cfg default 10 (cfg/TebLocalPlannerReconfigure.cfg:429-445) */
  /* robot_model (TebConfig::robot_model, teb_config.h:68) flattened */
  int32_t footprint_type;          /* TEB_AMD_FOOTPRINT_*                                              */
  double  footprint_radius;        /* circular: radius                                                 */
  double  footprint_front_offset;  /* two circles                                                      */
  double  footprint_front_radius;
  double  footprint_rear_offset;
  double  footprint_rear_radius;
  int32_t footprint_n_vertices;    /* line: 2 (start,end); polygon: >=1                                */
  double  footprint_vx[TEB_AMD_MAX_FOOTPRINT_VERTICES]; /* body-frame vertices                         */
  double  footprint_vy[TEB_AMD_MAX_FOOTPRINT_VERTICES];
  /* extension */
  int32_t jacobian_mode;           /* TEB_AMD_JACOBIAN_*                                               */
} teb_amd_config_t;

/*
 * Obstacle table (ObstContainer = std::vector<boost::shared_ptr<Obstacle>>, obstacles.h:262) as SoA.
 * All arrays have `count` entries except vert_offset (count+1, CSR) and vert_x/vert_y (vert_offset[count]).
 * vert_offset/vert_x/vert_y may be NULL when no TEB_AMD_OBST_POLYGON is present.
 * `dynamic` mirrors Obstacle::isDynamic() (set by setCentroidVelocity, obstacles.h:199-245).
 */
typedef struct teb_amd_obstacles {
  int32_t        count;
  const int32_t* type;
  const double*  ax;
  const double*  ay;
  const double*  bx;
  const double*  by;
  const double*  radius;
  const double*  vx;
  const double*  vy;
  const int32_t* dynamic;
  const int32_t* vert_offset;
  const double*  vert_x;
  const double*  vert_y;
} teb_amd_obstacles_t;

/*
 * A batch of B candidate TEBs (TebOptPlannerContainer, optimal_planner.h:702) as padded SoA:
 * pose i of TEB b lives at index b*stride + i. n[b] poses, n[b]-1 time differences.
 * First and last pose of every TEB are fixed (src/timed_elastic_band.cpp:330,377,398,442).
 * Per-TEB side inputs mirror TebOptimalPlanner members (optimal_planner.h:687-691):
 *   vel_start_ / vel_goal_ (pair<bool, Twist>: linear.x, linear.y, angular.z), prefer_rotdir_,
 *   and whether via_points_ is attached to this candidate (hcp.viapoints_all_candidates).
 */
typedef struct teb_amd_teb_batch {
  int32_t  count;      /* B */
  int32_t  stride;     /* >= max n[b]; <= max_poses of the handle */
  int32_t* n;          /* [B]   in: #poses; out (download): #poses after autoResize */
  double*  x;          /* [B*stride] */
  double*  y;
  double*  theta;
  double*  dt;         /* [B*stride]; dt[b*stride+i] connects pose i and i+1 */
  const int32_t* has_vel_start;   /* [B]  or NULL (= all 1: TebOptimalPlanner::initialize() fixes the start velocity,
                                   *      at zero until setVelocityStart, src/optimal_planner.cpp:94-97; 0 = free start
                                   *      velocity is an extension, the reference cannot express it) */
  const double*  vel_start;       /* [B*3] (vx, vy, omega) or NULL */
  const int32_t* has_vel_goal;    /* [B]  or NULL (= all 1, src/optimal_planner.cpp:99-102); 0 = setVelocityGoalFree() */
  const double*  vel_goal;        /* [B*3] or NULL */
  const int32_t* prefer_rotdir;   /* [B]  TEB_AMD_ROT_* or NULL (= none) */
  const int32_t* via_points_enabled; /* [B] or NULL (= all 1) */
} teb_amd_teb_batch_t;

/* Per-TEB outputs of one optimize_batch call. Any pointer may be NULL. */
typedef struct teb_amd_results {
  int32_t* status;         /* [B] TEB_AMD_TEB_*                                                       */
  int32_t* lm_iterations;  /* [B] LM iterations executed, summed over outer iterations (the "units")  */
  int32_t* lm_trials;      /* [B] damped-solve trials executed                                        */
  double*  chi2;           /* [B] chi^2 after the last LM iteration (g2o batchStatistics().back().chi2, */
                           /*     used by hasDiverged, src/optimal_planner.cpp:1023-1039)              */
  double*  cost;           /* [B] computeCurrentCost (src/optimal_planner.cpp:1041-1094); NaN if not asked */
  double*  lambda;         /* [B] final LM damping                                                     */
} teb_amd_results_t;

typedef struct teb_amd_handle teb_amd_handle_t;

/* -- library ------------------------------------------------------------------------------------ */
int  teb_amd_abi_version(void);
const char* teb_amd_last_error(void);           /* thread-local message of the last failing call */
void teb_amd_config_default(teb_amd_config_t* cfg);   /* TebConfig::TebConfig(), teb_config.h:245-390 */

/*
 * Behaviour switches of a handle (ABI 2; these were process-environment variables in ABI 1 - a library must not change its layout
 * because the host process happens to have a variable set). Zero-initialise, or teb_amd_options_default(), then override.
 */
enum { TEB_AMD_LAYOUT_AUTO = 0,        /* by capacity and obstacle count, and per launch by the current pose counts (see create) */
       TEB_AMD_LAYOUT_BLOCKS_LDS = 1,  /* normal matrix as 8x8 blocks in LDS, cyclic reduction in place (<= 238 poses)           */
       TEB_AMD_LAYOUT_BAND_LDS = 2,    /* band in LDS, cyclic reduction: level 0 from a band copy in HBM (<= 337 poses)         */
       TEB_AMD_LAYOUT_BAND_HBM = 3 };  /* band in HBM as well (<= TEB_AMD_MAX_POSES poses)                                      */
enum { TEB_AMD_HSIG3D_AUTO = 0, TEB_AMD_HSIG3D_WIDE = 1, TEB_AMD_HSIG3D_SMALL = 2 };
typedef struct teb_amd_options {
  int32_t struct_size;            /* sizeof(teb_amd_options_t) of the caller (forward compatibility); 0 = this header's         */
  int32_t layout;                 /* TEB_AMD_LAYOUT_*; anything but AUTO pins the layout (no per-launch choice)                 */
  int32_t fixed_layout;           /* 1: always launch in the capacity's own layout (no optimistic launch + repeat)              */
  int32_t band_ldlt;              /* 1: TEB_AMD_LAYOUT_BAND_LDS solves with the sequential banded LDL^T (cross-check, slow)     */
  int32_t generic_distance_path;  /* 1: never use the point-like LDS obstacle cache                                             */
  int32_t hsig3d_kernel;          /* TEB_AMD_HSIG3D_*: pin one of the two HSignature3d kernels                                  */
  int32_t no_near_cache;          /* 1: the near masks of the dynamic-obstacle edges are recomputed at every pass instead of    */
                                  /*    cached across one optimize() (cross-check: the results must not change by one bit)      */
  int32_t multi_cu;               /* small batches of generic-shape scenes on more than one CU (obstacle association and the       */
                                  /* robot <-> obstacle distances of every (pose, obstacle) pair are computed by helper workgroups */
                                  /* on the idle CUs, the bands are bit-identical to the single-CU result): 0 = automatic (ONE     */
                                  /* band, closed-form Jacobians, new association, enough obstacles x poses), -1 = never,         */
                                  /* n > 0 = at most n helper workgroups per band (and at most one per 6 poses of the capacity)    */
                                  /* on a batch of any size - with two or more bands and tens of helpers per band 0.05 - 2 % of    */
                                  /* the launches returned one band off the single-CU result (open defect). A launch with */
                                  /* distance helpers is synchronous and copies the strips first (it may have to be repeated); its */
                                  /* record buffer is bounded (1 GiB: beyond that, or when it cannot be allocated, the launch runs  */
                                  /* on one CU per band); misses are backed off, see teb_amd_multi_cu_backoff                       */
  int32_t multi_cu_timeout_us;    /* how long a band waits for its helper workgroups before it gives the launch up (it is then     */
                                  /* repeated on one CU per band); 0 = 2000 (2 ms: a phase takes some 10 us when the helpers have */
                                  /* CUs - they do unless other work occupies the device)                                          */
  int32_t speculative_trials;     /* small batches: the damped systems of the first retries of an LM iteration (lambda x 2, x 8,  */
                                  /* x 64) are solved on spare CUs while the band solves and evaluates its first trial, so that a  */
                                  /* rejected trial finds its step ready (bit-identical results): 0 = automatic (closed-form       */
                                  /* Jacobians, blocks-in-LDS or hybrid layout; as many of the three as the batch leaves CUs for:  */
                                  /* 3 solver workgroups per band up to 64 bands, 1 up to 128, none beyond), -1 = never,           */
                                  /* k = 1 .. 3: at most that many                                                                 */
  int32_t generic_config_path;    /* 1: never launch the kernel instantiations specialised on the TebConfig defaults. A configuration  */
                                  /* that takes the paths of a default TebConfig (non-holonomic, no via-points, new association, cost */
                                  /* exponent 1, no exact arc length, inflated obstacle edges, no batch statistics; point-like scenes: */
                                  /* diff-drive, point obstacles) runs kernels compiled with those flags folded: same operations,     */
                                  /* bit-identical bands, 10 - 25 % faster. Cross-check switch.                                        */
  int32_t compile_for_config;     /* a kernel compiled FOR the handle's configuration at run time (hipRTC, 2 - 5 s per instantiation, */
                                  /* cached per process and on disk): a configuration off the TebConfig defaults then runs a kernel  */
                                  /* with every flag of the profile table folded to ITS values - as fast as a default one,           */
                                  /* bit-identical bands. 0 = off, 1 = compile in the background at the first launch that needs it    */
                                  /* (the launches run the best pre-built kernel until the module is ready), 2 = that launch waits   */
                                  /* for the compiler. Needs libhiprtc and the ROCm headers ($ROCM_PATH, default /opt/rocm); the       */
                                  /* kernel sources are inside the library ($TEB_AMD_CSRC = a csrc directory to compile instead).     */
                                  /* Code objects are kept in $TEB_AMD_RTC_CACHE (default $XDG_CACHE_HOME/teb_amd or ~/.cache/teb_amd; */
                                  /* "off" = no disk cache), keyed by sources, flag values, instantiation and compiler version: the   */
                                  /* next process loads them in milliseconds. Where something is missing, or the compilation fails,   */
                                  /* the pre-built kernels run - it is never an error. The key holds scene-dependent flags too (via-  */
                                  /* points present, radii in the static list) and the layout of the launch: when one of them flips   */
                                  /* in a live planner, mode 1 runs the pre-built kernel until the new module is ready, mode 2 blocks  */
                                  /* that tick for the compiler - mode 2 is for benchmarks and tests, mode 1 for a robot. The disk    */
                                  /* cache is only used when its directory belongs to the calling user and nobody else can write it;  */
                                  /* its checksum detects corruption, it is no authentication.                                        */
  int32_t reserved[4];            /* must be 0                                                                                  */
} teb_amd_options_t;
void teb_amd_options_default(teb_amd_options_t* opt);

/*
 * create: one solver per GPU / host thread. device = HIP ordinal. stream = hipStream_t (as void*) to
 * launch on, or NULL for the handle's own stream. Fails (never falls back to CPU) when no gfx950 device.
 * max_poses = pose capacity of every band (trajectory.max_samples + 1 covers whatever autoResize can produce); up to
 * TEB_AMD_MAX_POSES (teb_amd_capacity). Layouts: normal matrix as 8x8 blocks in LDS up to 238 poses (208 beside a 500-obstacle cache) - the
 * fastest -, as a band in LDS up to 337, as a band in HBM beyond. Each launch uses the fastest layout that holds the current
 * bands with 10 % room to grow and is repeated in the capacity's own layout if autoResize outgrows that (teb_amd_options_t::fixed_layout:
 * always the capacity's layout); results do not depend on the layout.
 */
int  teb_amd_create(const teb_amd_config_t* cfg, int32_t max_tebs, int32_t max_poses,
                    int32_t max_obstacles, int32_t max_obstacle_vertices, int32_t max_via_points,
                    int32_t device, void* stream, teb_amd_handle_t** out);
/* the same with explicit options (NULL = defaults = teb_amd_create) */
int  teb_amd_create_ex(const teb_amd_config_t* cfg, int32_t max_tebs, int32_t max_poses,
                       int32_t max_obstacles, int32_t max_obstacle_vertices, int32_t max_via_points,
                       int32_t device, void* stream, const teb_amd_options_t* options, teb_amd_handle_t** out);
void teb_amd_destroy(teb_amd_handle_t* h);
/* dynamic_reconfigure. A change of include_dynamic_obstacles or of the footprint type re-derives the static / dynamic obstacle
 * lists and the distance path from the obstacle table the handle already holds (no re-upload needed). On an error (invalid
 * footprint / jacobian_mode) the handle keeps its previous configuration. */
int  teb_amd_set_config(teb_amd_handle_t* h, const teb_amd_config_t* cfg);

/* Scene, once per plan(): obstacles_ and via_points_ (optimal_planner.h:683-684). Host pointers. */
int  teb_amd_set_obstacles(teb_amd_handle_t* h, const teb_amd_obstacles_t* obst);
int  teb_amd_set_via_points(teb_amd_handle_t* h, int32_t count, const double* x, const double* y);

/* State strips host -> HBM and back. */
int  teb_amd_upload_tebs(teb_amd_handle_t* h, const teb_amd_teb_batch_t* batch);
int  teb_amd_download_tebs(teb_amd_handle_t* h, teb_amd_teb_batch_t* batch);

/*
 * The hot path: B x optimizeTEB (src/optimal_planner.cpp:182-231), i.e. optimizeAllTEBs
 * (src/homotopy_class_planner.cpp:466-493) when called with compute_cost=1 and the selection_* scales.
 * Asynchronous on the handle's stream; results are valid after teb_amd_synchronize / get_results. Two cases return only after the
 * launch has finished, because its per-band flags decide whether it has to be repeated: a handle launched in a faster layout than its
 * capacity's own (see teb_amd_create), and a launch with distance helpers (teb_amd_options_t::multi_cu).
 */
int  teb_amd_optimize_batch(teb_amd_handle_t* h, int32_t iterations_innerloop, int32_t iterations_outerloop,
                            int32_t compute_cost_afterwards, double obst_cost_scale,
                            double viapoint_cost_scale, int32_t alternative_time_cost);
int  teb_amd_synchronize(teb_amd_handle_t* h);
int  teb_amd_get_results(teb_amd_handle_t* h, teb_amd_results_t* out);   /* synchronises, copies D2H */

/*
 * Per-iteration log of the Levenberg-Marquardt loop, opt-in - the data of the line g2o prints per iteration when the reference sets
 * SparseOptimizer::setVerbose(cfg_->optim.optimization_verbose) (src/optimal_planner.cpp:384): "iteration= i chi2= .. lambda= ..
 * levenbergIter= ..". Row r (4 doubles) of band b describes LM iteration r of the last teb_amd_optimize_batch, counted over all outer
 * iterations: { chi^2 after the iteration (of the accepted state), lambda after it, damping trials the iteration took, pose count of
 * the band in that outer iteration }. At most TEB_AMD_ITERATION_LOG_ROWS rows per band are kept. Off by default (one extra store per
 * iteration and band when on). teb_amd_get_iteration_log synchronises; *n_rows = min(lm_iterations[b], capacity_rows, ROWS).
 */
#define TEB_AMD_ITERATION_LOG_ROWS 256
int  teb_amd_set_iteration_log(teb_amd_handle_t* h, int32_t enable);
int  teb_amd_get_iteration_log(teb_amd_handle_t* h, int32_t b, double* rows, int32_t capacity_rows, int32_t* n_rows);

/*
 * selectBestTeb (src/homotopy_class_planner.cpp:564-667) on the device-resident costs:
 * cost[last_best] *= selection_cost_hysteresis, cost[initial_plan] *= selection_prefer_initial_plan
 * (indices < 0 = none), strict '<' so the lowest index wins ties; TEBs whose status != OK still take
 * part exactly like in the reference (their stored cost_ is compared). Returns index in *best, its
 * (scaled) cost in *best_cost. The switching_blocking_period logic stays in the caller (needs ros::Time).
 */
int  teb_amd_select_best(teb_amd_handle_t* h, int32_t last_best, int32_t initial_plan,
                         int32_t* best, double* best_cost);

/* How the last teb_amd_optimize_batch ran: distance-helper and solver-helper workgroups per band of the multi-CU mode (0, 0 = one CU
 * per band), and whether the launch had to be repeated on one CU per band because the distance helpers did not arrive in time (a
 * device busy with other work). */
int  teb_amd_last_launch_info(teb_amd_handle_t* h, int32_t* distance_helpers_per_band, int32_t* solver_helpers_per_band,
                              int32_t* repeated_single_cu);
/* Back-off of the distance helpers on a device that is not empty: after a launch whose helpers came late (it was repeated on one CU per
 * band) the next *pause_length launches (4, doubling with every further miss up to 256) run on one CU per band without asking for
 * helpers - no wait, no repeat -, then one launch probes again; a probe that succeeds clears the pause. *launches_paused = how many of
 * them are still to come (0 = the next launch asks for helpers). A launch with distance helpers is synchronous (the per-band flags
 * decide about the repeat) and is preceded by a device-to-device copy of the strips; a paused one is neither. */
int  teb_amd_multi_cu_backoff(teb_amd_handle_t* h, int32_t* launches_paused, int32_t* pause_length);

/* -- zero-copy access for callers that already live on the GPU (benchmarks, torch interop) ---------- */
/*
 * f3 (candidate generation) — HomotopyClassPlanner::exploreEquivalenceClassesAndInitTebs after renewAndAnalyzeOldTebs
 * (src/homotopy_class_planner.cpp:318-340): GraphSearchInterface::createGraph (lrKeyPointGraph src/graph_search.cpp:95-223 when
 * simple_exploration, else ProbRoadmapGraph :227-340), the depth-first path enumeration (:45-91) and, for every start-goal path in
 * the reference's order, addAndInitNewTeb (homotopy_class_planner.hpp:66-93): band from the path (timed_elastic_band.hpp:46-183),
 * its equivalence class, addEquivalenceClassIfNew (src/homotopy_class_planner.cpp:189-212).
 */
typedef struct teb_amd_hcp_params {
  int32_t simple_exploration;                 /* hcp.simple_exploration: 1 = lrKeyPointGraph, 0 = ProbRoadmapGraph          */
  int32_t roadmap_graph_no_samples;           /* hcp.roadmap_graph_no_samples                                               */
  double  roadmap_graph_area_width;           /* hcp.roadmap_graph_area_width                                               */
  double  roadmap_graph_area_length_scale;    /* hcp.roadmap_graph_area_length_scale                                        */
  double  obstacle_heading_threshold;         /* hcp.obstacle_heading_threshold                                             */
  double  xy_goal_tolerance;                  /* goal_tolerance.xy_goal_tolerance                                           */
  int32_t max_number_classes;                 /* hcp.max_number_classes                                                     */
  int32_t max_number_plans_in_current_class;  /* hcp.max_number_plans_in_current_class                                      */
  double  h_signature_prescaler;              /* hcp.h_signature_prescaler                                                  */
  double  h_signature_threshold;              /* hcp.h_signature_threshold                                                  */
  int32_t allow_init_with_backwards_motion;   /* trajectory.allow_init_with_backwards_motion                                */
  int32_t delete_detours_backwards;           /* hcp.delete_detours_backwards                                               */
  double  detours_orientation_tolerance;      /* hcp.detours_orientation_tolerance                                          */
  double  length_start_orientation_vector;    /* hcp.length_start_orientation_vector                                        */
  double  max_ratio_detours_duration_best_duration; /* hcp.max_ratio_detours_duration_best_duration                        */
  int32_t global_plan_overwrite_orientation;  /* trajectory.global_plan_overwrite_orientation                               */
  int32_t viapoints_all_candidates;           /* hcp.viapoints_all_candidates                                               */
} teb_amd_hcp_params_t;
void teb_amd_hcp_params_default(teb_amd_hcp_params_t* p);   /* the defaults of teb_config.h:330-360 */
/*
 * The bands of the batch are the planner's tebs_ after renewAndAnalyzeOldTebs (teb_amd_compute_h_signatures,
 * teb_amd_filter_equivalence_classes, teb_amd_compact_bands; an empty batch is a planner without trajectories), best = index of
 * the last best band (its class may hold up to max_number_plans_in_current_class bands) or -1. New candidates are appended to the
 * batch while it holds fewer than max_number_classes (and than max_tebs) bands; *n_total = batch size afterwards.
 * start_vel = (linear.x, linear.y, angular.z) for setVelocityStart on the new bands or NULL; free_goal_vel = setVelocityGoalFree().
 * The collision tests of all vertex pairs against all obstacles, the band initialisation and the H-signatures of a chunk of
 * candidate paths run on the device; the depth-first enumeration (pointer chasing over the adjacency lists) runs on the host and
 * feeds the device in chunks of paths, which are accepted in the reference's order.
 * unit_samples: ProbRoadmapGraph only - [2*roadmap_graph_no_samples] uniform numbers in [0,1) replacing the planner's generator,
 * in draw order: per sample first the one scaled to the area width, then the one scaled to the area length (the order GCC gives
 * Eigen::Vector2d(distribution_x(g), distribution_y(g)), src/graph_search.cpp:274); NULL = the handle's own generator, the
 * default-seeded mt19937 + boost::random::uniform_real_distribution stream of the reference's member generator.
 * n_plan > 0: the initial plan of plan(initial_plan, ...) (positions and yaw of its poses; start / goal are its first / last pose):
 * it is tried as a candidate before the graph (addAndInitNewTeb(*initial_plan_, ...), src/homotopy_class_planner.cpp:326-329,
 * 412-440: band via initTrajectoryToGoal(plan, ...), its class is remembered as initial_plan_eq_class_). *initial_plan_teb =
 * getInitialPlanTEB() afterwards (:495-536): that band, else the first band of the remembered class, else -1 - the index to hand to
 * teb_amd_select_best. Via-points (updateReferenceTrajectoryViaPoints, :286-315): new candidates start without them; they are
 * enabled for all bands (viapoints_all_candidates) or, with an initial plan, for the bands of its class only.
 * *n_vertices / *n_paths (may be NULL): graph size and number of start-goal paths examined. max_paths > 0 bounds the enumeration
 * to that many start-goal paths and 10000 x max_paths vertex expansions (the reference has no bound: without new classes it
 * enumerates every simple path, and dead-end subtrees can be exponential in a large graph); TEB_AMD_OK is returned either way.
 */
int  teb_amd_explore_candidates(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const double* start, const double* goal,
                                double dist_to_obst, const double* start_vel, int32_t free_goal_vel, int32_t best,
                                const double* unit_samples, int64_t max_paths, int32_t* n_total, int32_t* n_vertices, int32_t* n_paths,
                                int32_t n_plan, const double* plan_x, const double* plan_y, const double* plan_yaw,
                                int32_t* initial_plan_teb);
/* the graph of the last teb_amd_explore_candidates call: vertices (x, y) [n_vertices], adjacency bytes [n_vertices^2] (row = from) */
int  teb_amd_get_exploration_graph(teb_amd_handle_t* h, double* vx, double* vy, unsigned char* adjacency, int32_t capacity_vertices,
                                   int32_t* n_vertices);
/*
 * Compaction of the batch after teb_amd_filter_equivalence_classes: the bands with keep[b] != 0 move to the front, in the order of
 * renewAndAnalyzeOldTebs (the last best band, best >= 0, swapped with the first one, src/homotopy_class_planner.cpp:220-224); the
 * batch shrinks to them. *n_kept = batch size afterwards, *new_best = position of the best band afterwards (0) or -1.
 */
int  teb_amd_compact_bands(teb_amd_handle_t* h, const int32_t* keep, int32_t best, int32_t* n_kept, int32_t* new_best);
/*
 * HomotopyClassPlanner::deletePlansDetouringBackwards (src/homotopy_class_planner.cpp:766-838), the second half of
 * renewAndAnalyzeOldTebs when hcp.delete_detours_backwards: keep [B] in/out - bands with keep[b] = 0 (erased by
 * teb_amd_filter_equivalence_classes) are not looked at; a remaining band other than the last best one (best) is dropped when it
 * has fewer than 2 poses, no pose further than length_start_orientation_vector from its start, a start direction more than
 * detours_orientation_tolerance away from the best band's, was not optimised by the last teb_amd_optimize_batch call
 * (TebOptimalPlanner::isOptimized), or lasts more than max_ratio_detours_duration_best_duration times the best band's duration.
 * Start directions and durations of all bands are computed in one launch. Call before teb_amd_compact_bands.
 */
int  teb_amd_filter_detours(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, int32_t best, int32_t* keep);
/* TebOptimalPlanner::optimized_ (optimal_planner.h:386, 691) of the resident bands: set by teb_amd_optimize_batch exactly as
 * optimizeTEB sets it (src/optimal_planner.cpp:189, 220), cleared by teb_amd_upload_tebs and for new bands; flags [B] overrides it
 * for bands whose history lives on the host (get: flags receives the current values). */
int  teb_amd_set_optimized_flags(teb_amd_handle_t* h, const int32_t* flags);
int  teb_amd_get_optimized_flags(teb_amd_handle_t* h, int32_t* flags);
/* per-band attributes of the resident batch, each [B], any may be NULL: via-points attached (TebOptimalPlanner::via_points_ != NULL),
 * vel_start_.first, vel_goal_.first */
int  teb_amd_get_band_flags(teb_amd_handle_t* h, int32_t* via_points_enabled, int32_t* has_vel_start, int32_t* has_vel_goal);
/* Device pointers (hipDeviceptr as void*) of the resident SoA strips: x, y, theta, dt, each
 * [max_tebs*max_poses] doubles, and n [max_tebs] int32. Valid until destroy.                          */
int  teb_amd_device_state(teb_amd_handle_t* h, void** x, void** y, void** theta, void** dt, void** n,
                          int32_t* stride);
/* Snapshot / restore the resident strips device-to-device (used to re-run identical work per step). */
int  teb_amd_snapshot_state(teb_amd_handle_t* h);
int  teb_amd_restore_state(teb_amd_handle_t* h);
/*
 * ---- Producers and consumers of the DEVICE-RESIDENT strips --------------------------------
 * With these a planning tick is: update_and_prune (or init_trajectory_*) -> set_obstacles -> optimize_batch -> select_best ->
 * get_velocity_command, without uploading or downloading the bands.
 *
 * f1 — TimedElasticBand::initTrajectoryToGoal, the three overloads, writing slot b (0 <= b < max_tebs; slots >= the current
 * batch size extend it, with the TebOptimalPlanner::initialize() defaults: start / goal velocity fixed at zero, no preferred turning
 * direction, via-points enabled). Poses are (x, y, theta). TEB_AMD_ERR_CAPACITY when the band would exceed max_poses.
 */
/* initTrajectoryToGoal(start, goal, diststep, max_vel_x, min_samples, guess_backwards_motion), src/timed_elastic_band.cpp:325-377 */
int  teb_amd_init_trajectory_line(teb_amd_handle_t* h, int32_t b, const double* start, const double* goal, double diststep,
                                  double max_vel_x, int32_t min_samples, int32_t guess_backwards_motion);
/* initTrajectoryToGoal(plan, max_vel_x, max_vel_theta, estimate_orient, min_samples, guess_backwards_motion), :380-452; the plan
 * (std::vector<geometry_msgs::PoseStamped>) as n_plan positions + yaw (tf::getYaw of each orientation) */
int  teb_amd_init_trajectory_plan(teb_amd_handle_t* h, int32_t b, int32_t n_plan, const double* plan_x, const double* plan_y,
                                  const double* plan_yaw, double max_vel_x, double max_vel_theta, int32_t estimate_orient,
                                  int32_t min_samples, int32_t guess_backwards_motion);
/* template initTrajectoryToGoal(path_start, path_end, fun_position, max_vel_x, max_vel_theta, max_acc_x, max_acc_theta,
 * start_orientation, goal_orientation, min_samples, guess_backwards_motion), timed_elastic_band.hpp:46-183 (the overload
 * HomotopyClassPlanner feeds with graph vertices). Optional arguments: NULL = boost::none. */
int  teb_amd_init_trajectory_path(teb_amd_handle_t* h, int32_t b, int32_t n_path, const double* path_x, const double* path_y,
                                  double max_vel_x, double max_vel_theta, const double* max_acc_x, const double* start_orientation,
                                  const double* goal_orientation, int32_t min_samples, int32_t guess_backwards_motion);
/* TimedElasticBand::updateAndPruneTEB(new_start, new_goal, min_samples), src/timed_elastic_band.cpp:555-597, on band b or on every
 * band of the batch (b = -1: HomotopyClassPlanner::updateAllTEBs, src/homotopy_class_planner.cpp:539-562). NULL = boost::none. */
int  teb_amd_update_and_prune(teb_amd_handle_t* h, int32_t b, const double* new_start, const double* new_goal, int32_t min_samples);
/* setVelocityStart / setVelocityGoal / setVelocityGoalFree (optimal_planner.h:247-260) on band b or all (b = -1);
 * fixed = 0 frees the velocity (the stored twist is kept), v = (linear.x, linear.y, angular.z) or NULL to keep the stored twist. */
int  teb_amd_set_velocity_start(teb_amd_handle_t* h, int32_t b, int32_t fixed, const double* v);
int  teb_amd_set_velocity_goal(teb_amd_handle_t* h, int32_t b, int32_t fixed, const double* v);
/* current pose counts of the batch (after init / prune / optimise), n [count] */
int  teb_amd_get_pose_counts(teb_amd_handle_t* h, int32_t* n, int32_t* count);
/*
 * f2 — consumers of the optimised strip of band b, computed on the device for the whole batch in one launch and cached until the
 * bands change: TebOptimalPlanner::getVelocityCommand (src/optimal_planner.cpp:1135-1168; *ok = its return value; uses
 * trajectory.prevent_look_ahead_poses_near_goal, passed here because teb_amd_config_t does not carry it), getVelocityProfile
 * (:1170-1196, out [(n+1)*3] = linear.x, linear.y, angular.z), getFullTrajectory (:1198-1247, out [n*7] = x, y, theta,
 * linear.x, linear.y, angular.z, time_from_start) and hasDiverged (:1023-1039).
 */
int  teb_amd_get_velocity_command(teb_amd_handle_t* h, int32_t b, int32_t look_ahead_poses,
                                  int32_t prevent_look_ahead_poses_near_goal, double* vx, double* vy, double* omega, int32_t* ok);
int  teb_amd_get_velocity_profile(teb_amd_handle_t* h, int32_t b, double* out, int32_t capacity_rows, int32_t* rows);
int  teb_amd_get_full_trajectory(teb_amd_handle_t* h, int32_t b, double* out, int32_t capacity_rows, int32_t* rows);
int  teb_amd_has_diverged(teb_amd_handle_t* h, int32_t b, int32_t* diverged);
/*
 * What optimizer_->batchStatistics() of every resident band would hold after the last teb_amd_optimize_batch (hasDiverged reads
 * .back().chi2, src/optimal_planner.cpp:1029-1038): available [count] = the vector is not empty (divergence_detection_enable was set
 * for that call, :331, and optimize() ran), back_chi2 [count] = .back().chi2. g2o sizes the vector to the REQUESTED inner iteration
 * count and fills one entry per executed iteration, so a band whose last optimize() call stopped early has back_chi2 = 0 and does not
 * count as diverged; teb_amd_has_diverged applies the same rule. A binding keeps the pair per planner object.
 */
int  teb_amd_get_batch_statistics(teb_amd_handle_t* h, int32_t* available, double* back_chi2);

/*
 * f4 (arithmetic part) — TebOptimalPlanner::isTrajectoryFeasible (src/optimal_planner.cpp:1250-1308; declared optimal_planner.h:500,
 * called by the ROS adapter at src/teb_local_planner_ros.cpp:396) on the device-resident bands. The costmap is the uint8 grid of
 * costmap_2d::Costmap2D (cells[my * size_x + mx]; 254 lethal, 253 inscribed, 255 no information; world (wx, wy) -> cell
 * ((int)((wx - origin_x) / resolution), (int)((wy - origin_y) / resolution))), uploaded once per tick; the footprint test is
 * base_local_planner::CostmapModel::footprintCost (outline rasterised with Bresenham; < 3 vertices: the centre cell) and, as in the
 * reference, only its value -1 (lethal) makes a pose infeasible - unknown cells and poses off the map do not.
 * footprint = footprint_spec [n_footprint <= 64] in the robot frame; inscribed_radius > 0 = robot_inscribed_radius_ (the adapter gets it
 * from costmap_2d::calculateMinAndMaxDistances); min_resolution_collision_check_angular = cfg.trajectory.<same>; look_ahead_idx =
 * cfg.trajectory.feasibility_check_no_poses (< 0 or >= n: the whole band); feasibility_check_lookahead_distance <= 0: off.
 * b >= 0: that band, outputs of 1 entry; b = -1: every band of the batch, outputs [B] (HomotopyClassPlanner checks its best band only,
 * src/homotopy_class_planner.cpp:727-737 - pass its index). first_infeasible (may be NULL): number of footprint tests that pass, in the
 * reference's order, before the colliding one; -1 if feasible. TEB_AMD_ERR_CAPACITY when the radii ask for more than 2^22 samples.
 */
int  teb_amd_set_costmap(teb_amd_handle_t* h, const uint8_t* cells, int32_t size_x, int32_t size_y, double resolution,
                         double origin_x, double origin_y);
int  teb_amd_is_trajectory_feasible(teb_amd_handle_t* h, int32_t b, int32_t n_footprint, const double* footprint_x,
                                    const double* footprint_y, double inscribed_radius, double min_resolution_collision_check_angular,
                                    int32_t look_ahead_idx, double feasibility_check_lookahead_distance, int32_t* feasible,
                                    int32_t* first_infeasible);

/*
 * The costmap's point obstacles, derived on the device — TebLocalPlannerROS::updateObstacleContainerWithCostmap
 * (src/teb_local_planner_ros.cpp:478-504; what computeVelocityCommands runs every tick when obstacles.include_costmap_obstacles, the
 * default, and no costmap converter is configured, :343-352) on the grid of the last teb_amd_set_costmap, followed by the caller's own
 * obstacles (what updateObstacleContainerWithCustomObstacles appends, :352), as the handle's obstacle table. The grid stays in the
 * handle: teb_amd_is_trajectory_feasible works on it afterwards as before.
 *   cells visited: mx = 0 .. size_x - 2 (outer loop), my = 0 .. size_y - 2 (inner loop) - the table is mx-major, the last column and
 *                  the last row are never visited, a grid with size_x == 1 or size_y == 1 yields no cell;
 *   cell counted:  cells[my * size_x + mx] == 254 (costmap_2d::LETHAL_OBSTACLE; 253 and 255 are not);
 *   centre:        wx = origin_x + (mx + 0.5) * resolution, wy likewise (costmap_2d::Costmap2D::mapToWorld);
 *   behind filter: (c, s) = (cos theta, sin theta) of robot_pose (PoseSE2::orientationUnitVec, pose_se2.h:215; std::cos / std::sin on
 *                  the host), d = (wx - x, wy - y); the cell is skipped iff d.x * c + d.y * s < 0 AND sqrt(d.x^2 + d.y^2) >
 *                  costmap_obstacles_behind_robot_dist (Eigen dot / norm of Vector2d: plain IEEE products and sums, correctly rounded
 *                  sqrt). A negative distance is allowed, as in the reference (src/teb_config.cpp:338 only warns).
 * The result is [n cell obstacles] ++ custom: every cell row TEB_AMD_OBST_POINT at the cell centre, radius 0, velocity 0, not dynamic.
 * Afterwards the handle behaves exactly as after teb_amd_set_obstacles with that concatenated table (lists, distance path and layout,
 * H-signature / exploration state, later teb_amd_set_config). robot_pose = (x, y, theta) of robot_pose_; custom may be NULL (no custom
 * obstacle). *n_costmap (may be NULL) receives n - also when the call fails with TEB_AMD_ERR_CAPACITY; out_x / out_y (may be NULL)
 * receive the first min(capacity, n) cell centres in table order (what a binding mirrors into its host ObstContainer).
 * Errors: no costmap set or a bad custom table -> TEB_AMD_ERR_INVALID_ARG; n + custom->count > max_obstacles or more polygon vertices
 * than max_obstacle_vertices -> TEB_AMD_ERR_CAPACITY. On every error the previous obstacle table and all that is derived from it are
 * left as they were.
 */
int  teb_amd_set_obstacles_from_costmap(teb_amd_handle_t* h, const double* robot_pose, double costmap_obstacles_behind_robot_dist,
                                        const teb_amd_obstacles_t* custom, int32_t* n_costmap, double* out_x, double* out_y,
                                        int32_t capacity);

/*
 * The costmap's lethal cells as a few convex obstacles, converted on the device — what computeVelocityCommands runs instead of the
 * point loop when obstacles.costmap_converter_plugin is set (teb_config.h:139; src/teb_local_planner_ros.cpp:345-349):
 * updateObstacleContainerWithCostmapConverter (:506-549) over the polygons a converter makes from the grid of the last
 * teb_amd_set_costmap, followed by the caller's own obstacles (:352), as the handle's obstacle table. The conversion rule:
 *   cells kept:  exactly those teb_amd_set_obstacles_from_costmap keeps (same visit domain, value 254 only, same behind filter; a
 *                distance of +inf switches the filter off);
 *   tiles:       T = tile_cells (1 .. 64); tile (tx, ty) covers mx in [tx*T, tx*T + T), my in [ty*T, ty*T + T), clipped to the visit
 *                domain; components are the 8-connected kept cells of one tile (they never cross a tile border, which bounds the
 *                over-approximation: a hull of whole rows of walls would cover the room between them);
 *   row:         the convex hull of a component's cell indices (mx, my), Andrew's monotone chain on integers with strict turns only
 *                (no vertex collinear with its neighbours): 1 vertex -> TEB_AMD_OBST_POINT; 2 -> TEB_AMD_OBST_LINE from the
 *                lexicographically smallest to the largest (mx, my); 3 or more -> TEB_AMD_OBST_POLYGON, counter-clockwise from the
 *                lexicographically smallest vertex, no repeated closing vertex (the reference's 1 / 2 / more vertices cases);
 *   vertex:      cell (mx, my) at (origin_x + (mx + 0.5) * resolution, origin_y + (my + 0.5) * resolution), the point route's bits;
 *                radius 0, velocity 0, not dynamic; centroids and bounding radii as teb_amd_set_obstacles derives them;
 *   order:       tiles tx outer, ty inner (the point route's cell order); inside a tile by the smallest (mx, my) cell of the
 *                component; then the custom rows.
 * With T = 1 the table is the one teb_amd_set_obstacles_from_costmap makes; every kept cell centre lies in the closed hull of its row.
 * Afterwards the handle behaves exactly as after teb_amd_set_obstacles with [converted rows] ++ custom (lists, distance path and
 * layout, H-signature / exploration state, later teb_amd_set_config). robot_pose = (x, y, theta); custom may be NULL.
 * *n_obstacles and *n_points (each may be NULL) receive the number of converted rows and of their vertices (every row's, ObstacleMsg
 * style) - also when the call fails with TEB_AMD_ERR_CAPACITY. out_offset [capacity_obstacles + 1], out_x / out_y [capacity_points]
 * (may be NULL) receive the converted rows as a polygon list - row i has the vertices out_offset[i] .. out_offset[i + 1] - 1 - what a
 * binding mirrors into its host ObstContainer; they are written only when n_obstacles <= capacity_obstacles and n_points <=
 * capacity_points.
 * Errors: no costmap set, tile_cells outside 1 .. 64, a negative capacity, a null pose or a bad custom table -> TEB_AMD_ERR_INVALID_ARG;
 * converted rows + custom->count > max_obstacles, or converted polygon vertices + custom polygon vertices > max_obstacle_vertices ->
 * TEB_AMD_ERR_CAPACITY. On every error the previous obstacle table and all that is derived from it are left as they were.
 */
int  teb_amd_set_obstacles_from_costmap_polygons(teb_amd_handle_t* h, const double* robot_pose,
                                                 double costmap_obstacles_behind_robot_dist, int32_t tile_cells,
                                                 const teb_amd_obstacles_t* custom, int32_t* n_obstacles, int32_t* n_points,
                                                 int32_t* out_offset, double* out_x, double* out_y, int32_t capacity_obstacles,
                                                 int32_t capacity_points);

/*
 * f3 (arithmetic core) — equivalence classes of the device-resident bands, as HomotopyClassPlanner::calculateEquivalenceClass
 * (homotopy_class_planner.hpp:46-62) computes them for every candidate in renewAndAnalyzeOldTebs: HSignature3d
 * (h_signature.h:281-347; one value per obstacle) when cfg.include_dynamic_obstacles, else HSignature (h_signature.h:96-188; one
 * complex value). One launch for the whole batch. prescaler = hcp.h_signature_prescaler. values (may be NULL): 3-D [B*M] in
 * obstacle-table order, 2-D [B*2] = (re, im). *width receives M or 2.
 */
int  teb_amd_compute_h_signatures(teb_amd_handle_t* h, double prescaler, double* values, int32_t* width);
/*
 * The class list of renewAndAnalyzeOldTebs / addEquivalenceClassIfNew / hasEquivalenceClass (src/homotopy_class_planner.cpp:178-254)
 * over the signatures of the last teb_amd_compute_h_signatures call: bands are visited in order, with the last best band first
 * (best >= 0; std::iter_swap with the first band); keep[b] = 1 iff band b opens a new class or is one of at most
 * max_number_plans_in_current_class bands in the best band's class; valid[b] = isValid(), reasonable[b] = isReasonable()
 * (h_signature.h:190-226, 349-409). threshold = hcp.h_signature_threshold. Output arrays [B], any may be NULL.
 */
int  teb_amd_filter_equivalence_classes(teb_amd_handle_t* h, double threshold, int32_t best, int32_t max_number_plans_in_current_class,
                                        int32_t* keep, int32_t* valid, int32_t* reasonable);

/*
 * ---- Multi-GPU: one process per GPU, the candidate batch sharded by contiguous blocks, scene replicated, no
 * data-path collective. The path's single exchange - best-trajectory selection - lives here, behind the C-ABI, so that the C++
 * drop-in (HomotopyClassPlannerAmd) can shard as well: an RCCL communicator over xGMI (librccl is dlopen'ed on first use).
 *   rank 0:    teb_amd_comm_unique_id(id)            -> ship the 128 bytes to the other ranks by any means (MPI, a ROS param, a file,
 *                                                        torch.distributed)
 *   all ranks: teb_amd_comm_create(id, rank, world, device, &comm)
 *   per plan:  teb_amd_optimize_batch(h, ...)         each rank on its own candidates
 *              teb_amd_select_best_distributed(...)    one ncclAllGather of 16 bytes per rank; same answer on every rank
 *              teb_amd_broadcast_band(...)             optional: the winner's strip (24 + 32 * capacity bytes) from its owner to all
 */
#define TEB_AMD_COMM_ID_BYTES 128
typedef struct teb_amd_comm teb_amd_comm_t;
int  teb_amd_comm_unique_id(char id[TEB_AMD_COMM_ID_BYTES]);
int  teb_amd_comm_create(const char id[TEB_AMD_COMM_ID_BYTES], int32_t rank, int32_t world, int32_t device, teb_amd_comm_t** out);
void teb_amd_comm_destroy(teb_amd_comm_t* comm);
/*
 * selectBestTeb (src/homotopy_class_planner.cpp:564-667) over the candidates of ALL ranks. This rank holds the global candidates
 * [global_offset, global_offset + B); last_best_global / initial_plan_global are global indices (< 0 = none) and receive the
 * hysteresis / prefer-initial-plan multipliers on the rank that owns them. Lowest cost wins, ties -> lowest global index (strict '<'
 * of :610). *best_global, *best_cost (scaled, bit-exact: costs travel as fp64), *owner_rank are identical on every rank.
 * Collective: every rank of the communicator must call it. Runs on the handle's stream and synchronises it.
 */
int  teb_amd_select_best_distributed(teb_amd_handle_t* h, teb_amd_comm_t* comm, int32_t global_offset, int32_t last_best_global,
                                     int32_t initial_plan_global, int32_t* best_global, double* best_cost, int32_t* owner_rank);
/*
 * The winner's strip from its owner to every rank (host buffers x, y, theta, dt of `capacity` doubles each, *n poses): what the rank
 * that talks to the robot needs for getVelocityCommand / visualisation. local_index is only read on owner_rank. capacity must be
 * the same on every rank and >= the winner's pose count (TEB_AMD_ERR_CAPACITY otherwise, on every rank). Collective.
 */
int  teb_amd_broadcast_band(teb_amd_handle_t* h, teb_amd_comm_t* comm, int32_t owner_rank, int32_t local_index, int32_t capacity,
                            int32_t* n, double* x, double* y, double* theta, double* dt);
/*
 * The winner's batch statistics travel with its strip (24 bytes more): what teb_amd_get_batch_statistics returns for the band on its
 * owner, as received by the last teb_amd_broadcast_band on this communicator. A rank that mirrors the winner answers hasDiverged
 * (src/optimal_planner.cpp:1023-1039; the plugin asks after every plan(), src/teb_local_planner_ros.cpp:374) like the owner does.
 */
int  teb_amd_comm_last_band_statistics(const teb_amd_comm_t* comm, int32_t* available, double* back_chi2);

/* Duration [ms] of the last optimize_batch call on the device, measured with HIP events on the launch stream: from before the
 * (first) kernel launch to after the last one, i.e. including a repeated launch when autoResize outgrew the optimistic layout. */
int  teb_amd_last_kernel_ms(teb_amd_handle_t* h, float* ms);
/* Shader clock [MHz] the last optimise kernel ran at: shader-cycle counter / 100 MHz real-time counter between entry and exit of its
 * first workgroup. The boxes of a pool sustain different clocks under the same load; a measurement quotes it so that a slow box is not
 * read as a regression. */
int  teb_amd_last_shader_clock_mhz(teb_amd_handle_t* h, double* mhz);
/* LDS bytes per workgroup and the largest pose count this build can optimise. */
int  teb_amd_capacity(teb_amd_handle_t* h, int32_t* lds_bytes, int32_t* max_poses_supported);

/*
 * ---- Fleet batches: the bands of many scenes in ONE launch -----------------------------------------------------------------------
 * A handle can hold a SET of scenes (an obstacle table and a via-point list each) and a band -> scene map; teb_amd_optimize_batch then
 * runs every band against its own scene, one workgroup per band, one launch. Many robots with a few candidates each fill the device
 * the way one robot's candidates cannot. Without a class map (teb_amd_set_scene_configs, below) every scene runs under the handle's
 * configuration and footprint; with one, every scene runs under the configuration of its robot class (a heterogeneous fleet).
 *
 * Contract: every band ends with the bits it has in a single-scene handle that is created with the configuration of the band's scene
 * (the handle's own without a class map, else that of the scene's class), holds only the band's scene, has the same capacities and
 * layout and the options generic_config_path = 1, multi_cu = -1, speculative_trials = -1 - provided that handle runs the same
 * distance path as the fleet: the point-like path iff the rows of EVERY scene and the footprint of EVERY class are point-like and the
 * LDS cache of the largest scene fits, the generic one otherwise (a point-like scene or robot inside a generic fleet equals its
 * handle with generic_distance_path = 1).
 *
 * Robot classes - a configuration and a footprint per scene. A robot class is one teb_amd_config_t, footprint included; the class map
 * gives every scene of the set its class. Valid only while scenes are set.
 *   teb_amd_set_scene_configs  installs n_classes >= 1 configurations and class_of_scene [n_scenes]; n_scenes must be the number of
 *                            scenes set and every entry lie in [0, n_classes). Every configuration passes the checks of
 *                            teb_amd_set_config. These fields must agree over the classes of one map, because one decision of the
 *                            host covers the whole launch: jacobian_mode (TEB_AMD_JACOBIAN_ANALYTIC: fleet kernels exist for
 *                            closed-form Jacobians) and include_dynamic_obstacles (the 2-D / 3-D kind of the per-scene signature
 *                            calls is one per launch). What teb_amd_optimize_batch takes as arguments is one value per launch
 *                            whatever the classes hold: the iteration counts, and for the costs of the bands obst_cost_scale,
 *                            viapoint_cost_scale and alternative_time_cost - a caller who takes them from a configuration
 *                            (selection_obst_cost_scale, selection_viapoint_cost_scale, selection_alternative_time_cost) passes
 *                            ONE class's values, and the costs of every band are scaled by them;
 *                            teb_amd_optimize_batch_per_class reads them from the class of every band instead.
 *                            TEB_AMD_ERR_INVALID_ARG names the class and the field. Everything
 *                            is checked before anything live is touched: on any error - a layout that cannot be had with the new
 *                            footprints included - the previous map, or none, stays installed and the handle behaves as if the call
 *                            had not been made. The lists of every scene are derived from its class; classes need not be used.
 *                            The map has the lifetime of the scene count, like the remembered best class of a scene: kept across
 *                            teb_amd_set_scenes and the two costmap routes when they install the same number of scenes (the new
 *                            tables' lists are derived per class), forgotten by teb_amd_clear_scenes, by a set of another size and
 *                            by teb_amd_clear_scene_configs. While a map is installed, fleet launches and the per-band rules below
 *                            ignore the handle's own configuration; teb_amd_set_config still changes it - for single-scene mode
 *                            and for after the map is cleared - and leaves the map alone.
 *   teb_amd_clear_scene_configs  back to the handle's configuration for every scene. No map installed: no effect.
 *   teb_amd_get_scene_configs  *n_classes (0 = no map; may be NULL); class_of_scene NULL: count only, else the class of every scene
 *                            (capacity < n_scenes: TEB_AMD_ERR_CAPACITY).
 * One class equal to the handle's configuration gives the bits of the same fleet without a map. What takes the class of the band's
 * scene: the optimise launch, the lists teb_amd_set_scenes* derives, the consumers (velocity command, profile, full trajectory),
 * teb_amd_select_best_per_scene (selection_cost_hysteresis, selection_prefer_initial_plan), teb_amd_has_diverged and
 * teb_amd_get_batch_statistics (divergence_detection_*). A launch may change the pose counts when ANY class has teb_autosize. What
 * reads nothing else of the configuration and works unchanged: the signature, class-filter, detour and compaction calls per scene.
 * Limits: while a map with MORE THAN ONE class is installed, teb_amd_explore_candidates_per_scene returns TEB_AMD_ERR_UNSUPPORTED -
 * it takes max_vel_x, max_vel_theta, acc_lim_x, min_samples and weight_viapoint from ONE configuration and dist_to_obst as one value
 * per call (with one class it runs under that class); teb_amd_explore_candidates_per_class takes its place.
 * teb_amd_is_trajectory_feasible_per_scene keeps its one footprint per call; teb_amd_is_trajectory_feasible_per_class takes one per spec.
 *
 * The whole tick per class - the _per_class calls. One naming rule: a _per_class call is its _per_scene sibling (or
 * teb_amd_optimize_batch) WITHOUT every argument that stands for a configuration field; it reads those fields for scene s from the
 * configuration of the scene's class, and without a class map from the handle's configuration (the table of one class the fleet launch
 * uses). Valid only while scenes are set, else TEB_AMD_ERR_INVALID_ARG, like their siblings. Everything the sibling documents holds.
 *   teb_amd_explore_candidates_per_class  teb_amd_explore_candidates_per_scene without dist_to_obst. For scene s of class k:
 *                            min_obstacle_dist is the graph's dist_to_obst (vertices and edges); max_vel_x, max_vel_theta, min_samples
 *                            initialise the bands made from initial plans; max_vel_x, acc_lim_x, min_samples the path bands; max_vel_x,
 *                            min_samples the at-goal line bands; weight_viapoint decides the via-point rule after the tick.
 *                            teb_amd_hcp_params_t stays one per call. Contract: the bands of scene s, read in band order, are bit for
 *                            bit the batch of a single-scene handle that is created with class k's configuration, holds only scene s,
 *                            held the same bands before the call and ran teb_amd_explore_candidates with dist_to_obst =
 *                            min_obstacle_dist of class k and the arguments of s - bands, flags, n_vertices, n_paths, graph,
 *                            initial_plan_teb and the order of the tail of the batch. Generators, remembered classes and last graphs
 *                            are the per-scene state of teb_amd_explore_candidates_per_scene, shared with it.
 *   teb_amd_update_and_prune_per_class  teb_amd_update_and_prune_per_scene without min_samples: every band is pruned with min_samples
 *                            of its scene's class.
 *   teb_amd_optimize_batch_per_class  teb_amd_optimize_batch where band b takes obst_cost_scale, viapoint_cost_scale and
 *                            alternative_time_cost from selection_obst_cost_scale, selection_viapoint_cost_scale and
 *                            selection_alternative_time_cost of its scene's class. Layout, refusals and the repeat after an optimistic
 *                            layout are those of teb_amd_optimize_batch; the iteration counts stay arguments. Every band ends with the
 *                            bits of teb_amd_optimize_batch with any triple; its cost has the bits of its single-scene handle (contract
 *                            above) launched with its class's triple.
 *   teb_amd_is_trajectory_feasible_per_class  teb_amd_is_trajectory_feasible_per_scene with a teb_amd_feasibility_spec_t - footprint,
 *                            inscribed radius, angular resolution, look-ahead pair - per scene: spec_of_scene[s] in [0, n_specs), or
 *                            NULL = the class of scene s, which needs n_specs = the number of classes of the map (1 without a map).
 *                            Every spec passes the checks of the single call (1 <= n_footprint <= 64, radius and angular resolution
 *                            > 0); TEB_AMD_ERR_INVALID_ARG names the spec. One launch, one download. The pair of scene s is what
 *                            teb_amd_is_trajectory_feasible(bands[s]) gives with its spec on a handle whose costmap is grid s. The band,
 *                            scene and costmap-set refusals and the sample and pose limits are those of the per-scene call.
 *
 *   teb_amd_set_scenes       installs n_scenes scenes (1 <= n_scenes <= max_tebs) and enters fleet mode. The fleet storage is a second
 *                            set of device buffers, allocated at the first call and sized by the handle's capacities: sum of the rows
 *                            <= max_obstacles, sum of the polygon vertices <= max_obstacle_vertices, sum of the via-points <=
 *                            max_via_points. via_count NULL = no via-points; via_x / via_y hold the lists of the scenes one after the
 *                            other. Everything is parsed and checked before the first upload: on an argument or capacity error
 *                            (the codes of teb_amd_set_obstacles) the previous scene set stays installed. Only a device error
 *                            during the upload itself (TEB_AMD_ERR_HIP) leaves the handle in single-scene mode, without a scene
 *                            set. The single-scene table, its lists, its layout choice and its H-signatures are not touched.
 *   teb_amd_set_band_scenes  scene of band 0 .. count - 1; bands >= count belong to scene 0, as every band does before the first call.
 *                            The map belongs to the handle: it survives teb_amd_set_scenes and teb_amd_clear_scenes, and
 *                            teb_amd_compact_bands moves its entries with the bands (the slots it frees go back to scene 0).
 *                            teb_amd_optimize_batch returns TEB_AMD_ERR_INVALID_ARG when a band maps to a scene >= n_scenes, or when
 *                            jacobian_mode is TEB_AMD_JACOBIAN_G2O_NUMERIC (fleet kernels exist for closed-form Jacobians).
 *   teb_amd_get_band_scenes  the map of the resident bands as compaction and per-scene exploration moved and extended it: *count = B
 *                            (may be NULL); scene_of NULL: count only; capacity < B: TEB_AMD_ERR_CAPACITY.
 *   teb_amd_clear_scenes     back to the single-scene table as it was.
 *   teb_amd_get_scene_count  0 = single-scene mode.
 *   teb_amd_select_best_per_scene  teb_amd_select_best over the bands of every scene: last_best / initial_plan [n_scenes] are BAND
 *                            indices or -1 (NULL = none); best[s] = band index, -1 for a scene without bands; best_cost [n_scenes] may
 *                            be NULL.
 *
 * A fleet launch has no helper workgroups, is never compiled at run time and follows the layout rules of teb_amd_optimize_batch (the
 * optimistic layout and its repeat use the largest scene). teb_amd_set_config re-derives the lists of every scene (without a class map;
 * with one the lists follow the classes and the call leaves them alone). Everything that
 * works on band b without the scene works unchanged (the three initialisers, update_and_prune, velocities, consumers, feasibility,
 * results, upload / download, snapshot / restore, teb_amd_compact_bands). The calls that read or write THE scene of the handle return
 * TEB_AMD_ERR_INVALID_ARG while scenes are set (call teb_amd_clear_scenes first): teb_amd_set_obstacles, both costmap routes,
 * teb_amd_set_via_points, teb_amd_compute_h_signatures / teb_amd_filter_equivalence_classes / teb_amd_filter_detours (their
 * per-scene forms below take their place), teb_amd_explore_candidates (teb_amd_explore_candidates_per_scene takes its place),
 * teb_amd_select_best and the distributed calls (a refused rank still enters the collective and sends the unusable record, as for
 * any other error of one rank), teb_amd_debug_linearize, teb_amd_debug_distance. Product library only (the other build variants
 * refuse the launch).
 *
 * Equivalence classes per scene - renewAndAnalyzeOldTebs of every robot of the fleet. Valid only while scenes are set; in single-scene
 * mode the three calls return TEB_AMD_ERR_INVALID_ARG (call teb_amd_set_scenes first).
 *   teb_amd_compute_h_signatures_per_scene  teb_amd_compute_h_signatures of every band against its OWN scene, in one launch: a
 *                            band's values are the bits of a single-scene handle that holds only its scene. Values lie band after
 *                            band; band b holds offset[b + 1] - offset[b] of them: the row count of its scene when
 *                            cfg.include_dynamic_obstacles (a scene without rows: none), else 2 = (re, im) ((0, 0) for a scene without
 *                            rows). offset [B + 1] may be NULL. *n_values (may be NULL) always receives the total. values NULL:
 *                            compute only. Otherwise values is written when capacity_values >= *n_values, and the call returns
 *                            TEB_AMD_ERR_CAPACITY when not - the signatures are computed and kept for the filter call either way.
 *                            A band that maps to a scene >= n_scenes: TEB_AMD_ERR_INVALID_ARG, as for teb_amd_optimize_batch.
 *                            teb_amd_options_t::hsig3d_kernel pins the 3-D kernel as for the single scene.
 *   teb_amd_filter_equivalence_classes_per_scene  the rule of teb_amd_filter_equivalence_classes over the bands of every scene in
 *                            band order, scene by scene: best [n_scenes] (NULL = none) holds a band of scene s, visited first, or a
 *                            negative value; a band of another scene is TEB_AMD_ERR_INVALID_ARG. Every scene remembers its own best
 *                            class (a planner is a robot is a scene): it is kept across teb_amd_set_scenes calls with the same
 *                            number of scenes, used only when its kind and width match the scene's signatures, and forgotten by
 *                            teb_amd_clear_scenes or another number of scenes. keep / valid / reasonable [B], any may be NULL.
 *                            Without valid signatures: TEB_AMD_ERR_INVALID_ARG (compute first).
 *   teb_amd_filter_detours_per_scene  the rule of teb_amd_filter_detours scene by scene after ONE statistics launch over all bands;
 *                            every scene has its own early-out (fewer than two kept bands, best[s] negative or not kept).
 * The per-scene signatures, their validity and the 2-D products of the set are state of the scene set: teb_amd_set_scenes,
 * teb_amd_set_band_scenes, teb_amd_clear_scenes, teb_amd_set_config, teb_amd_compact_bands and every call that changes the bands
 * invalidate them. None of the three touches the single scene's state: after teb_amd_clear_scenes, teb_amd_compute_h_signatures and
 * teb_amd_filter_equivalence_classes give what they gave before teb_amd_set_scenes, remembered best class included.
 *
 * Candidate exploration per scene - exploreEquivalenceClassesAndInitTebs of every robot of the fleet. Valid only while scenes are set;
 * in single-scene mode the three calls return TEB_AMD_ERR_INVALID_ARG (call teb_amd_set_scenes first). Every output pointer may be NULL.
 *   teb_amd_explore_candidates_per_scene  teb_amd_explore_candidates of every scene with its own start / goal [3 n_scenes], start
 *                            velocity [3 n_scenes] or NULL, best band (best[s]: a band of scene s or negative, NULL = none; a band of
 *                            another scene is TEB_AMD_ERR_INVALID_ARG), unit samples ([n_scenes][2 roadmap_graph_no_samples] or NULL)
 *                            and initial plan (plan_count [n_scenes] or NULL = none; the poses of the plans one after the other in
 *                            plan_x / plan_y / plan_yaw). Contract: the bands of scene s, read in band order, are bit for bit the batch
 *                            of a single-scene handle that holds only scene s, held the same bands of s before the call and ran
 *                            teb_amd_explore_candidates with the arguments of s (max_tebs >= max_number_classes there): number and
 *                            order of the bands, x / y / theta / dt, the via-point / velocity flags, n_vertices[s], n_paths[s], the
 *                            graph, and initial_plan_teb[s] - the position of that band AMONG THE BANDS OF SCENE s, or -1.
 *                            n_bands[s] = bands of scene s after the call, *n_total = all bands. New bands are appended to the batch
 *                            and enter the band -> scene map. Their order at the tail: first the bands made from the initial plans, by
 *                            scene index; then round by round the accepted graph candidates, by scene index and within a scene in
 *                            path order (a round takes up to a fixed number of paths from every scene that still has room; the bands
 *                            of a scene and every count are independent of that number); last the line bands of the scenes that
 *                            stand at their goal without a band, by scene index.
 *                            Every scene has its own default-seeded generator for the roadmap samples, its own remembered best class
 *                            (shared with teb_amd_filter_equivalence_classes_per_scene), remembered initial-plan class and last graph:
 *                            kept across teb_amd_set_scenes calls with the same number of scenes, forgotten by teb_amd_clear_scenes or
 *                            another number of scenes. A scene that returns before its graph (full, or start within xy_goal_tolerance
 *                            of the goal) draws nothing. None of this touches the single scene's state, generator included.
 *                            Capacity: with c_s bands of scene s before the call, sum_s max(c_s, max_number_classes) > max_tebs
 *                            returns TEB_AMD_ERR_CAPACITY before anything changes. A start-goal path or plan longer than a band:
 *                            TEB_AMD_ERR_CAPACITY as for the single scene; the bands accepted so far stay and the map matches them.
 *                            A band that maps to a scene >= n_scenes: TEB_AMD_ERR_INVALID_ARG. The per-scene signatures are reused
 *                            when they are fresh (same bands, same prescaler) and are stale after the call.
 *   teb_amd_get_exploration_graph_per_scene  teb_amd_get_exploration_graph for the last graph of one scene (*n_vertices = 0: the scene
 *                            returned before its graph in the last call).
 *   teb_amd_compact_bands_per_scene  within every scene the band best[s] and the scene's first band exchange places (std::iter_swap of
 *                            renewAndAnalyzeOldTebs); then the kept bands move to the front of the batch in that order, the map with
 *                            them (freed slots: scene 0). For every scene the subsequence of its bands is what
 *                            teb_amd_compact_bands(keep of s, best of s) leaves on a handle that holds only that scene. new_best[s] =
 *                            new index of the scene's best band, -1 when it was dropped or none was given. *n_kept = bands left.
 *
 * Both ends of a fleet tick per scene - the costmaps in, the checks and the commands out. A costmap set holds one grid per scene.
 *   teb_amd_set_costmaps     n grids of any sizes, `cells` one grid after the other (row-major, size_x[s] * size_y[s] bytes each), in one
 *                            device buffer; grid s belongs to scene s. State of the handle BESIDE the single costmap of
 *                            teb_amd_set_costmap, which is not touched and still serves the single-scene calls. n = 0 drops the set.
 *                            Everything is checked before the first upload: on a bad argument (n < 0, a null array, a size <= 0, a
 *                            resolution that is not > 0; n > max_tebs: TEB_AMD_ERR_CAPACITY) the previous set stays.
 *   teb_amd_set_scenes_from_costmaps  teb_amd_set_scenes with table s = the rows teb_amd_set_obstacles_from_costmap makes from grid s
 *                            and robot_pose[3 s .. 3 s + 3) (the reference's column-major order) ++ the rows of custom[s] (custom NULL:
 *                            none anywhere). Three launches serve all scenes (count, scan, write), the host reads n_scenes totals and
 *                            then the points once. Needs a costmap set with n = n_scenes, else TEB_AMD_ERR_INVALID_ARG. n_costmap
 *                            [n_scenes] (or NULL) = cell rows of every scene, also when the call then fails with TEB_AMD_ERR_CAPACITY
 *                            because the sum of the cell rows and the custom rows exceeds max_obstacles; out_x / out_y (or NULL): the
 *                            cell centres of the scenes one after the other, at most `capacity` of them. An argument or capacity error
 *                            leaves the previous scene set installed.
 *   teb_amd_set_scenes_from_costmap_polygons  teb_amd_set_scenes with table s = the rows teb_amd_set_obstacles_from_costmap_polygons
 *                            makes from grid s, robot_pose[3 s .. 3 s + 3) and tile_cells[s] (same conversion rule, row order, vertex
 *                            bits, derived centroids and radii) ++ the rows of custom[s] (custom NULL: none anywhere). The tile size is
 *                            per scene: sparse maps want 1, structured maps 8, and a fleet has both. Three launches serve all scenes
 *                            (count, scan, write: as many workgroups as the scenes have blocks together), the host reads the
 *                            3 n_scenes totals and then the offsets and vertices once. Needs a costmap set with n = n_scenes. A grid
 *                            without a visit domain (size_x < 2 or size_y < 2) converts to no rows. n_obstacles / n_points [n_scenes]
 *                            (or NULL) = converted rows of every scene and their vertices, also when the call then fails with
 *                            TEB_AMD_ERR_CAPACITY. out_offset [capacity_obstacles + 1], out_x / out_y [capacity_points] (or NULL): the
 *                            polygon list of the scenes one after the other - row i of the concatenation has the vertices
 *                            out_offset[i] .. out_offset[i + 1] - 1 of the concatenated arrays, (sum of rows) + 1 offsets; written
 *                            only when all three are given, the sum of the rows <= capacity_obstacles and the sum of the vertices <=
 *                            capacity_points. TEB_AMD_ERR_INVALID_ARG: n_scenes < 1, a null pose array, null tile_cells, a tile size
 *                            outside 1 .. 64, a negative capacity, a costmap set of another size, a bad custom table, bad via
 *                            arrays. TEB_AMD_ERR_CAPACITY: converted + custom rows > max_obstacles, converted + custom polygon
 *                            vertices > max_obstacle_vertices, via-points > max_via_points, grids too large for one call. Everything
 *                            is checked before the live scene set is touched: on these errors the previous set stays installed and
 *                            behaves as if the call had not been made. teb_amd_set_obstacles_from_costmap_polygons itself stays a
 *                            single-scene call (refused while scenes are set).
 *   teb_amd_is_trajectory_feasible_per_scene  teb_amd_is_trajectory_feasible of ONE band per scene against the scene's own grid, in
 *                            one launch with one download: bands[s] is a band of scene s, or negative - then feasible[s] =
 *                            first_infeasible[s] = -1. The pair of scene s is what teb_amd_is_trajectory_feasible(bands[s]) gives on a
 *                            handle whose costmap is grid s. TEB_AMD_ERR_INVALID_ARG: a band of another scene, a band index >= the
 *                            number of bands, no scenes set, a costmap set whose size is not the number of scenes. The sample limit and
 *                            the 1024-pose limit are those of the single call.
 *   teb_amd_update_and_prune_per_scene  teb_amd_update_and_prune of every band with the start / goal of ITS scene (new_start /
 *                            new_goal [3 n_scenes], NULL: leave it), in one launch; where start_vel [3 n_scenes] is given and
 *                            has_start_vel[s] != 0 (NULL: every scene) the bands of scene s get what teb_amd_set_velocity_start(b, 1,
 *                            start_vel + 3 s) leaves. The call does not wait for the kernel. Invalidates what teb_amd_update_and_prune
 *                            invalidates, and the per-scene signatures. TEB_AMD_ERR_INVALID_ARG: no scenes set, a band that maps to a
 *                            scene >= n_scenes, no bands.
 *   teb_amd_get_velocity_commands  teb_amd_get_velocity_command of n bands after one launch and one download: cmd [n][3] = (vx, vy,
 *                            omega), ok [n]; a negative band gives ok = 0 and zeros. Available in either mode.
 */
int  teb_amd_set_scenes(teb_amd_handle_t* h, int32_t n_scenes, const teb_amd_obstacles_t* obstacles /* [n_scenes] */,
                        const int32_t* via_count /* [n_scenes] or NULL */, const double* via_x, const double* via_y /* concatenated */);
int  teb_amd_set_band_scenes(teb_amd_handle_t* h, const int32_t* scene_of, int32_t count);
int  teb_amd_get_band_scenes(teb_amd_handle_t* h, int32_t* scene_of /* [capacity] or NULL */, int32_t capacity, int32_t* count);
int  teb_amd_clear_scenes(teb_amd_handle_t* h);
int  teb_amd_get_scene_count(teb_amd_handle_t* h, int32_t* n_scenes);
int  teb_amd_set_scene_configs(teb_amd_handle_t* h, int32_t n_classes, const teb_amd_config_t* configs /* [n_classes] */,
                               int32_t n_scenes, const int32_t* class_of_scene /* [n_scenes] */);
int  teb_amd_clear_scene_configs(teb_amd_handle_t* h);
int  teb_amd_get_scene_configs(teb_amd_handle_t* h, int32_t* n_classes, int32_t* class_of_scene /* [capacity] or NULL */,
                               int32_t capacity);
int  teb_amd_select_best_per_scene(teb_amd_handle_t* h, const int32_t* last_best, const int32_t* initial_plan,
                                   int32_t* best /* [n_scenes] */, double* best_cost);
int  teb_amd_compute_h_signatures_per_scene(teb_amd_handle_t* h, double prescaler, double* values, int64_t capacity_values,
                                            int32_t* offset /* [B + 1] or NULL */, int64_t* n_values);
int  teb_amd_filter_equivalence_classes_per_scene(teb_amd_handle_t* h, double threshold,
                                                  const int32_t* best /* [n_scenes] band index or -1; NULL = none */,
                                                  int32_t max_number_plans_in_current_class, int32_t* keep, int32_t* valid,
                                                  int32_t* reasonable /* [B], any may be NULL */);
int  teb_amd_filter_detours_per_scene(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const int32_t* best /* [n_scenes] */,
                                      int32_t* keep /* [B] in/out */);
int  teb_amd_explore_candidates_per_scene(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const double* start /* [3 n_scenes] */,
                                          const double* goal /* [3 n_scenes] */, double dist_to_obst,
                                          const double* start_vel /* [3 n_scenes] or NULL */, int32_t free_goal_vel,
                                          const int32_t* best /* [n_scenes] band of scene s or negative; NULL = none */,
                                          const double* unit_samples /* [n_scenes][2 roadmap_graph_no_samples] or NULL */,
                                          int64_t max_paths, int32_t* n_total, int32_t* n_bands /* [n_scenes] */,
                                          int32_t* n_vertices /* [n_scenes] */, int32_t* n_paths /* [n_scenes] */,
                                          const int32_t* plan_count /* [n_scenes] or NULL */, const double* plan_x, const double* plan_y,
                                          const double* plan_yaw /* concatenated */, int32_t* initial_plan_teb /* [n_scenes] */);
int  teb_amd_get_exploration_graph_per_scene(teb_amd_handle_t* h, int32_t scene, double* vx, double* vy, unsigned char* adjacency,
                                             int32_t capacity_vertices, int32_t* n_vertices);
int  teb_amd_compact_bands_per_scene(teb_amd_handle_t* h, const int32_t* keep /* [B] */, const int32_t* best /* [n_scenes] or NULL */,
                                     int32_t* n_kept, int32_t* new_best /* [n_scenes] */);
int  teb_amd_set_costmaps(teb_amd_handle_t* h, int32_t n, const uint8_t* cells /* grids one after the other, row-major */,
                          const int32_t* size_x, const int32_t* size_y, const double* resolution, const double* origin_x,
                          const double* origin_y /* [n] each */);
int  teb_amd_set_scenes_from_costmaps(teb_amd_handle_t* h, int32_t n_scenes, const double* robot_pose /* [3 n_scenes] */,
                                      double costmap_obstacles_behind_robot_dist, const teb_amd_obstacles_t* custom /* [n_scenes] or NULL */,
                                      const int32_t* via_count /* [n_scenes] or NULL */, const double* via_x, const double* via_y,
                                      int32_t* n_costmap /* [n_scenes] or NULL */, double* out_x, double* out_y /* concatenated, or NULL */,
                                      int32_t capacity);
int  teb_amd_set_scenes_from_costmap_polygons(teb_amd_handle_t* h, int32_t n_scenes, const double* robot_pose /* [3 n_scenes] */,
                                              double costmap_obstacles_behind_robot_dist, const int32_t* tile_cells /* [n_scenes], each 1 .. 64 */,
                                              const teb_amd_obstacles_t* custom /* [n_scenes] or NULL */, const int32_t* via_count,
                                              const double* via_x, const double* via_y, int32_t* n_obstacles /* [n_scenes] or NULL */,
                                              int32_t* n_points /* [n_scenes] or NULL */, int32_t* out_offset, double* out_x, double* out_y,
                                              int32_t capacity_obstacles, int32_t capacity_points);
int  teb_amd_is_trajectory_feasible_per_scene(teb_amd_handle_t* h, const int32_t* bands /* [n_scenes]: a band of scene s, or negative */,
                                              int32_t n_footprint, const double* footprint_x, const double* footprint_y,
                                              double inscribed_radius, double min_resolution_collision_check_angular,
                                              int32_t look_ahead_idx, double feasibility_check_lookahead_distance,
                                              int32_t* feasible /* [n_scenes] */, int32_t* first_infeasible /* [n_scenes] or NULL */);
int  teb_amd_update_and_prune_per_scene(teb_amd_handle_t* h, const double* new_start /* [3 n_scenes] or NULL */,
                                        const double* new_goal /* [3 n_scenes] or NULL */, int32_t min_samples,
                                        const double* start_vel /* [3 n_scenes] or NULL */,
                                        const int32_t* has_start_vel /* [n_scenes] or NULL = all */);
/* the _per_class calls (above: the whole tick per class) */
typedef struct teb_amd_feasibility_spec {      /* what the adapter passes to isTrajectoryFeasible for one robot class */
  int32_t n_footprint; const double* footprint_x; const double* footprint_y;
  double  inscribed_radius, min_resolution_collision_check_angular;
  int32_t look_ahead_idx; double feasibility_check_lookahead_distance;
} teb_amd_feasibility_spec_t;
int  teb_amd_explore_candidates_per_class(teb_amd_handle_t* h, const teb_amd_hcp_params_t* p, const double* start /* [3 n_scenes] */,
                                          const double* goal /* [3 n_scenes] */, const double* start_vel /* [3 n_scenes] or NULL */,
                                          int32_t free_goal_vel, const int32_t* best /* [n_scenes] band of scene s or negative; NULL = none */,
                                          const double* unit_samples /* [n_scenes][2 roadmap_graph_no_samples] or NULL */,
                                          int64_t max_paths, int32_t* n_total, int32_t* n_bands /* [n_scenes] */,
                                          int32_t* n_vertices /* [n_scenes] */, int32_t* n_paths /* [n_scenes] */,
                                          const int32_t* plan_count /* [n_scenes] or NULL */, const double* plan_x, const double* plan_y,
                                          const double* plan_yaw /* concatenated */, int32_t* initial_plan_teb /* [n_scenes] */);
int  teb_amd_update_and_prune_per_class(teb_amd_handle_t* h, const double* new_start /* [3 n_scenes] or NULL */,
                                        const double* new_goal /* [3 n_scenes] or NULL */,
                                        const double* start_vel /* [3 n_scenes] or NULL */,
                                        const int32_t* has_start_vel /* [n_scenes] or NULL = all */);
int  teb_amd_optimize_batch_per_class(teb_amd_handle_t* h, int32_t iterations_innerloop, int32_t iterations_outerloop,
                                      int32_t compute_cost_afterwards);
int  teb_amd_is_trajectory_feasible_per_class(teb_amd_handle_t* h, const int32_t* bands /* [n_scenes] */, int32_t n_specs,
                                              const teb_amd_feasibility_spec_t* specs,
                                              const int32_t* spec_of_scene /* [n_scenes]; NULL = the class map's class_of_scene */,
                                              int32_t* feasible, int32_t* first_infeasible /* [n_scenes] or NULL */);
int  teb_amd_get_velocity_commands(teb_amd_handle_t* h, int32_t n, const int32_t* bands /* [n], negative = none */,
                                   int32_t look_ahead_poses, int32_t prevent_look_ahead_poses_near_goal, double* cmd /* [n][3] */,
                                   int32_t* ok /* [n] */);

/*
 * ---- Local plan windows per robot from resident global plans ---------------------------------------------------------------------------
 * What TebLocalPlannerROS::computeVelocityCommands derives from the robot's global plan and pose before it calls plan()
 * (src/teb_local_planner_ros.cpp:268-340): pruneGlobalPlan (:657-698), transformGlobalPlan (:701-822), updateViaPointsContainer
 * (:627-645), estimateLocalGoalOrientation (:827-871), the start replacement (:336-340) and the transformed global goal of the
 * goal-reached test (:291-292) - for every robot of a fleet in ONE launch (csrc/teb_plan_window.hpp: one workgroup per robot). The
 * global plans live on the device like the costmaps; per tick only the poses go in. tf is the caller's: the plan -> global transform
 * arrives as five doubles (cos, sin, tx, ty, yaw_tf), cos and sin computed on the host, so the device transform is products and sums.
 * Every index and count is the reference's sequential decision bit for bit; positions and copied yaws are plain IEEE products and sums.
 *
 * The parameters are the four of cfg_.trajectory the adapter reads (teb_config.h:259-264) and the moving_average_length default of
 * estimateLocalGoalOrientation (teb_local_planner_ros.h); they are no part of teb_amd_config_t.
 */
typedef struct teb_amd_plan_window_params {
  int32_t struct_size;                        /* sizeof(teb_amd_plan_window_params_t), set by teb_amd_plan_window_params_default  */
  double  global_plan_prune_distance;         /* 1                                                                                */
  double  max_global_plan_lookahead_dist;     /* 1; <= 0: no length cut                                                           */
  double  global_plan_viapoint_sep;           /* -1; <= 0: no via-points                                                          */
  int32_t global_plan_overwrite_orientation;  /* 1                                                                                */
  int32_t moving_average_length;              /* 3                                                                                */
} teb_amd_plan_window_params_t;
void teb_amd_plan_window_params_default(teb_amd_plan_window_params_t* p);
int  teb_amd_sizeof_plan_window_params(void);
/*
 *   teb_amd_set_global_plans  n plans, plan r = plan_count[r] poses (x, y, yaw) in the plan frame, the plans one after the other in
 *                            x / y / yaw; ONE device buffer, sized by the call. begin [n] (NULL = zeros) is the pruning cursor of every
 *                            robot: what pruneGlobalPlan has erased so far; a caller that replaces one robot's plan passes the other
 *                            robots' cursors (teb_amd_get_plan_cursors) to keep them. State of the handle beside the costmap set and
 *                            the scene set: it touches neither and is valid in single-scene and fleet mode. n = 0 drops the set.
 *                            TEB_AMD_ERR_CAPACITY: n > max_tebs. TEB_AMD_ERR_INVALID_ARG: n < 0, null plan_count, a count < 0, a cursor
 *                            outside 0 .. count, a null array while the counts sum to more than 0. Everything is checked before the
 *                            first upload: on an argument or capacity error, or a failed device allocation, the previous set
 *                            stays. A device error during the upload itself (TEB_AMD_ERR_HIP) leaves the handle without a set.
 *   teb_amd_plan_windows     the windows of all n robots (n = size of the plan set, else TEB_AMD_ERR_INVALID_ARG; so is a call without
 *                            a set, null robot_pose / dist_threshold, a params struct of another size, a negative capacity).
 *                            robot_pose [3 n] = (x, y, theta) in the global frame; plan_to_global [5 n] or NULL = identity;
 *                            dist_threshold [n] = the reference's 0.85 * max(size_x, size_y) * resolution / 2 of every robot's costmap
 *                            (:729-731). params NULL = the defaults. Steps per robot, every index relative to the cursor:
 *                              robot in the plan frame  R^T (g - t);
 *                              prune      first pose with squared distance < prune_distance^2 becomes the cursor (pruned = 1); none:
 *                                         the cursor stays, pruned = 0;
 *                              closest    i = first index of the minimum squared distance over the poses scanned; the scan ends at the
 *                                         first pose farther than the running minimum once that minimum is < 0.05 (a loop in the
 *                                         path: the first local minimum wins); sq_dist starts at 1e10;
 *                              window     poses i .. k_end - 1: pose k is taken while the previous squared distance <= dist_threshold^2
 *                                         and (lookahead <= 0 or plan_length <= lookahead), plan_length += |p(k-1) p(k)| after pose k
 *                                         (k > 0), summed in that order; goal_idx = k_end - 1; an empty window: the global goal alone,
 *                                         goal_idx = N - 1;
 *                              transform  R p + t; yaw unchanged when yaw_tf == 0, else g2o::normalize_theta(yaw + yaw_tf);
 *                              via-points from the last accepted pose (first: pose 0 of the window) the first later pose at distance
 *                                         >= global_plan_viapoint_sep, on the transformed window before its first pose is replaced;
 *                              goal       position of the window's last pose; yaw, when global_plan_overwrite_orientation: its own
 *                                         (goal_idx >= N - 1), the global goal's transformed yaw (goal_idx > N - moving_average_length
 *                                         - 2), else average_angles of up to moving_average_length headings between consecutive
 *                                         transformed poses after goal_idx; the window's last yaw becomes the goal yaw;
 *                              start      a one-pose window gets a pose inserted in front; pose 0 becomes robot_pose.
 *                            Outputs per robot, each may be NULL: window_count [n] (poses of the delivered window, start insertion
 *                            included), goal_idx [n], cursor [n] (the new begin, also kept on the device for the next call), pruned
 *                            [n], goal [3 n], global_goal [3 n] (the plan's last pose, transformed), via_count [n]; offset [n + 1] with
 *                            win_x / win_y / win_yaw [capacity_window] and via_offset [n + 1] with via_x / via_y [capacity_via]: the
 *                            windows / via-points of the robots one after the other. Counts, offsets and per-robot values are always
 *                            delivered; the concatenated arrays are written only when they fit, otherwise the call returns
 *                            TEB_AMD_ERR_CAPACITY (the cursors have moved all the same). One launch; one download for the per-robot
 *                            records, one for the arrays. A robot with an empty plan (count 0, or a cursor at its end) returns
 *                            window_count = 0, goal_idx = 0, pruned = 1 and zeros.
 *   teb_amd_get_plan_cursors begin [n of the set]; without a set TEB_AMD_ERR_INVALID_ARG.
 * All three refuse a null handle with TEB_AMD_ERR_INVALID_ARG before touching it, and are part of every library variant.
 */
int  teb_amd_set_global_plans(teb_amd_handle_t* h, int32_t n, const int32_t* plan_count /* [n] */, const double* x, const double* y,
                              const double* yaw /* concatenated */, const int32_t* begin /* [n] or NULL = 0 */);
int  teb_amd_plan_windows(teb_amd_handle_t* h, int32_t n, const teb_amd_plan_window_params_t* params, const double* robot_pose /* [3 n] */,
                          const double* plan_to_global /* [5 n] or NULL */, const double* dist_threshold /* [n] */,
                          int32_t* window_count, int32_t* goal_idx, int32_t* cursor, int32_t* pruned /* [n] each */,
                          double* goal /* [3 n] */, double* global_goal /* [3 n] */, int32_t* via_count /* [n] */,
                          int32_t* offset /* [n + 1] */, double* win_x, double* win_y, double* win_yaw, int32_t capacity_window,
                          int32_t* via_offset /* [n + 1] */, double* via_x, double* via_y, int32_t capacity_via);
int  teb_amd_get_plan_cursors(teb_amd_handle_t* h, int32_t* begin /* [n] */);

#ifdef __cplusplus
}
#endif
#endif /* TEB_AMD_H_ */
