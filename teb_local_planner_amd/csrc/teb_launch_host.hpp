// teb_launch_host.hpp — what a teb_amd_optimize_batch call launches: the host policy of the optimise launch, each decision stated once
// as a pure function of a few integers, free of HIP: the layout of a handle at create, of an obstacle table, of one launch; the helper
// workgroups of the multi-CU mode and their back-off; what follows a look at the per-band flags (the repeat ladder); which
// instantiation of the kernel runs. The LDS plan enters only as a callable bytes(S, layout, cache entries) - teb_amd.hip passes
// make_lds_plan(..).total_bytes, tests/host/launch_host_check.cpp a synthetic one with thresholds that can be worked out by hand. The
// launches, allocations, copies and synchronisations are the driver's (teb_amd.hip: teb_amd_create_ex, choose_scene_layout, launch,
// launch_opt, rtc_lookup).
#pragma once

#include <algorithm>
#include <cstddef>

#include "../../include/teb_amd.h"

namespace tebamd {

// The layouts of the normal matrix and the scene kinds of the instantiations by the numbers the kernel headers give them (teb_kernel.hpp:
// SOLVER_*, SCENE_*; teb_amd.hip asserts that they are the same).
enum { LAYOUT_BAND = 0, LAYOUT_BLOCKS = 1, LAYOUT_BAND_HBM = 2 };
enum { KIND_NONE = -1, KIND_POINTS = 0, KIND_GENERIC = 1, KIND_POINTS_SMALL = 2, KIND_GENERIC_SMALL = 3, KIND_POINTS_DEFAULTS = 4,
       KIND_POINTS_SMALL_DEFAULTS = 5, KIND_GENERIC_DEFAULTS = 6, KIND_GENERIC_SMALL_DEFAULTS = 7, KIND_POINTS_WIDE = 8,
       KIND_POINTS_SMALL_WIDE = 9, KIND_POINTS_LIGHT = 10, KIND_POINTS_SMALL_LIGHT = 11, KIND_POINTS_CUSTOM = 12,
       KIND_POINTS_SMALL_CUSTOM = 13, KIND_GENERIC_CUSTOM = 14, KIND_GENERIC_SMALL_CUSTOM = 15 };
constexpr int kMaxSolverHelpers = 3;   // teb_multicu.hpp: kMcuMaxSpec
constexpr int kBlocksMaxPoses = 238, kLdsBandMaxPoses = 337;   // the longest band each LDS layout holds on a full workgroup's LDS

// ---- layout at create ------------------------------------------------------------------------------------------------------------------
struct CreateLayout {
  enum Refused { NO = 0, BLOCKS_TOO_LARGE, CAPACITY };
  int layout = LAYOUT_BLOCKS;
  Refused refused = NO;
  size_t lds = 0;         // CAPACITY: what max_poses needs in that layout ..
  int thread_limit = 0;   // .. and the poses a workgroup's lanes hold in it
};
// Normal matrix as 8x8 blocks in LDS (LAYOUT_BLOCKS: cyclic reduction in place, fastest) when that fits TOGETHER with the LDS cache
// of a full obstacle table of max_obstacles point-like entries; otherwise as a band in LDS (LAYOUT_BAND: 44 instead of 70
// doubles per pose) with the hybrid cyclic reduction (level 0 from a band-form copy in HBM) - within 2 % of the block layout
// per step, keeps the obstacle cache and holds bands up to 337 poses. pin: teb_amd_options_t::layout.
template <class PlanBytes>
CreateLayout layout_at_create(int max_poses, int max_obstacles, size_t lds_limit, int pin, int threads, int pose_iter_band_hbm, PlanBytes bytes) {
  const int ob = max_obstacles > 0 ? max_obstacles : 0;
  CreateLayout r;
  if (bytes(max_poses, LAYOUT_BLOCKS, 0) > lds_limit) r.layout = LAYOUT_BAND;
  else if (bytes(max_poses, LAYOUT_BLOCKS, ob) > lds_limit && bytes(max_poses, LAYOUT_BAND, ob) <= lds_limit) r.layout = LAYOUT_BAND;
  if (pin == TEB_AMD_LAYOUT_BAND_LDS) r.layout = LAYOUT_BAND;
  else if (pin == TEB_AMD_LAYOUT_BAND_HBM) r.layout = LAYOUT_BAND_HBM;
  else if (pin == TEB_AMD_LAYOUT_BLOCKS_LDS) {
    if (bytes(max_poses, LAYOUT_BLOCKS, 0) > lds_limit) { r.refused = CreateLayout::BLOCKS_TOO_LARGE; return r; }
    r.layout = LAYOUT_BLOCKS;
  }
  // bands too long for the LDS band (> 337 poses; the reference's max_samples default is 500): the band form of the normal matrix
  // moves to HBM (LAYOUT_BAND_HBM: 44 doubles per pose, L2-resident), everything else stays as it is
  if (r.layout == LAYOUT_BAND && bytes(max_poses, LAYOUT_BAND, 0) > lds_limit) r.layout = LAYOUT_BAND_HBM;
  // more than two poses per lane: only the band-in-HBM instantiations are compiled for it (teb_device.hpp: kPoseIterBandHbm)
  if (max_poses > threads * 2) r.layout = LAYOUT_BAND_HBM;   // (the LDS layouts end at 337 poses: the checks above have already moved it there)
  r.lds = bytes(max_poses, r.layout, 0);
  r.thread_limit = threads * (r.layout == LAYOUT_BAND_HBM ? pose_iter_band_hbm : 2);
  if (max_poses > r.thread_limit || r.lds > lds_limit) r.refused = CreateLayout::CAPACITY;
  return r;
}

// ---- layout per obstacle table ---------------------------------------------------------------------------------------------------------
struct TableLayout {
  int layout = 0;
  int fast_points = 0;     // the point-like distance path with its LDS cache
  int cache_entries = 0;   // what the LDS plan of the table is made for: M with fast_points, else 0
  bool hbm_band = false;   // the band moved to HBM: the handle needs its per-band HBM band buffer
};
// The distance path and the layout that goes with it, for an obstacle cache of M entries (the widest table): point-like fast path iff all
// obstacles are Point/Circular, the footprint is Point/Circular, and the cache fits the LDS. created: the layout of the handle; pin:
// teb_amd_options_t::layout; stride: the pose capacity.
template <class PlanBytes>
TableLayout layout_per_table(bool pointlike_rows, int footprint_type, bool generic_distance_path, int created, int pin, int M, int stride,
                             size_t lds_limit, PlanBytes bytes) {
  bool pointlike = pointlike_rows && (footprint_type == TEB_AMD_FOOTPRINT_POINT || footprint_type == TEB_AMD_FOOTPRINT_CIRCULAR);
  if (generic_distance_path) pointlike = false;
  TableLayout t;
  t.layout = created;
  // a point-like scene whose obstacle cache does not fit beside the LDS band: the band moves to HBM and the cache stays (measured,
  // 64 bands x 337 poses x 500 obstacles: 9.0 instead of 11.8 ms per step)
  if (pointlike && M > 0 && created == LAYOUT_BAND && pin == TEB_AMD_LAYOUT_AUTO && bytes(stride, LAYOUT_BAND, M) > lds_limit &&
      bytes(stride, LAYOUT_BAND_HBM, M) <= lds_limit) {
    t.layout = LAYOUT_BAND_HBM;
    t.hbm_band = true;
  }
  if (pointlike && M > 0 && bytes(stride, t.layout, M) <= lds_limit) { t.fast_points = 1; t.cache_entries = M; }
  return t;
}

// ---- layout per launch -----------------------------------------------------------------------------------------------------------------
// largest pose capacity <= upto whose LDS plan (with the obstacle cache of this scene, if it is in use) fits; 0: none down to 8 poses
template <class PlanBytes>
int max_capacity_of(int layout, int upto, int cache_entries, size_t lds_limit, PlanBytes bytes) {
  int S = upto;
  while (S > 8 && bytes(S, layout, cache_entries) > lds_limit) --S;
  return bytes(S, layout, cache_entries) <= lds_limit ? S : 0;
}
// The four switches that keep a launch in the handle's own layout: the debug launch of one linearisation, teb_amd_options_t::fixed_layout,
// a pinned teb_amd_options_t::layout, the sequential banded LDL^T.
struct LayoutSwitches {
  bool debug_linearize, fixed_layout, pinned, band_ldlt;
};
// (the driver asks first: only then does it need the pose counts, which may cost a read-back)
inline bool may_launch_optimistic(int own, const LayoutSwitches& sw) {
  return own != LAYOUT_BLOCKS && !sw.debug_linearize && !sw.fixed_layout && !sw.pinned && !sw.band_ldlt;
}
struct LaunchLayout {
  int layout, S;     // optimistic: the plan is made for S poses (and the same cache entries); else the table's own plan
  bool optimistic;
};
// The layout of the normal matrix follows the pose capacity of the handle (blocks in LDS <= 238 poses, band in LDS <= 337, band in
// HBM beyond), the faster layouts only hold shorter bands. A handle created for long bands that currently holds short ones is
// launched in the fastest layout that leaves the bands 10 % room to grow (autoResize); should a band outgrow it all the same, the
// launch is repeated from the saved strips in the handle's own layout (after_first_look). Results do not depend on the layout (same
// arithmetic up to the order of the block reduction). nmax: the longest resident band.
template <class PlanBytes>
LaunchLayout layout_per_launch(int own, const LayoutSwitches& sw, int nmax, int stride, int cache_entries, size_t lds_limit, PlanBytes bytes) {
  if (may_launch_optimistic(own, sw)) {
    const int need = nmax + nmax / 10 + 4;   // 10 % room to grow; a band that needs more triggers the repeat
    const int s_blocks = max_capacity_of(LAYOUT_BLOCKS, std::min(stride, kBlocksMaxPoses), cache_entries, lds_limit, bytes);
    if (s_blocks > 0 && need <= s_blocks) return LaunchLayout{LAYOUT_BLOCKS, s_blocks, true};
    const int s_band = own == LAYOUT_BAND_HBM ? max_capacity_of(LAYOUT_BAND, std::min(stride, kLdsBandMaxPoses), cache_entries, lds_limit, bytes) : 0;
    if (s_band > 0 && need <= s_band) return LaunchLayout{LAYOUT_BAND, s_band, true};
  }
  return LaunchLayout{own, stride, false};
}

// ---- helper workgroups -----------------------------------------------------------------------------------------------------------------
// Back-off of the distance helpers: after a launch whose helpers came late (a device busy with other work) the next
// `left` launches run on one CU per band without asking; then one launch probes again. Every further miss doubles the pause
// (4, 8, .. 256 launches), a probe that succeeds clears it.
struct HelperBackoff {
  int left = 0, len = 0;
  // paused after a miss: this launch runs on one CU per band, no wait, no repeat
  bool consume_paused_launch() {
    if (left <= 0) return false;
    --left;
    return true;
  }
  // after a launch with distance helpers whose flags were read
  void update(bool helpers_late) {
    len = helpers_late ? std::min(256, std::max(4, 2 * len)) : 0;
    left = len;
  }
  // a probe after a pause waits 250 us at most: helpers that have CUs answer a phase within ~ 10 us, and a device that is still busy
  // should cost the tick as little as possible beyond its one-CU time
  long long probe_timeout(long long ticks) const { return len > 0 ? std::min(ticks, 25000LL) : ticks; }
};
// how long a band waits for its helpers, in ticks of the 100 MHz real-time counter (teb_amd_options_t::multi_cu_timeout_us, 0: 2 ms)
inline long long helper_timeout_ticks(int timeout_us) { return (long long)(timeout_us > 0 ? timeout_us : 2000) * 100LL; }

constexpr size_t kMcuItemsMaxBytes = (size_t)1 << 30;   // distance records of the multi-CU mode: beyond 1 GiB the launch stays on one CU per band
// distance records [B][M][4][stride]: bounded (the association list of a pose is short, but its capacity is every obstacle)
inline size_t distance_records(int B, int M, int stride) { return (size_t)B * M * 4 * stride; }

struct HelperInputs {
  bool fleet;                // the launch runs against a scene set
  bool debug_linearize;
  int jacobian_mode;         // TEB_AMD_JACOBIAN_*
  int B, M, stride;          // bands, obstacles of the scene, pose capacity
  int nmax_known;            // the longest resident band as far as the host knows, <= 0: unknown
  int num_cus;               // <= 0: unknown (256)
  int speculative_trials, multi_cu;   // teb_amd_options_t
  int layout;                // of this launch
  bool band_ldlt;
  int inner;                 // iterations of the inner loop
  bool fast_points;          // point-like scene
  bool legacy_association;   // teb_amd_config_t::legacy_obstacle_association
};
struct Helpers {
  int K = 0, D = 0;   // solver / distance helpers per band
};
// Multi-CU mode (teb_multicu.hpp): helper workgroups per band of this launch - K solver helpers (speculative LM trials, any scene kind)
// and D distance helpers (generic scenes: association + distance records). Small batches only: one workgroup per CU (the LDS footprint
// of the layouts) means B (1 + K + D) <= number of CUs keeps every workgroup resident. Closed-form Jacobians (the small-batch
// instantiations); the solver helpers need a layout whose normal matrix another workgroup can pick up (blocks in LDS with their HBM
// backup, or the band copy of the hybrid solve), the distance helpers the new association. A fleet launch has no helper workgroups.
inline Helpers helpers_wanted(const HelperInputs& in) {
  Helpers r;
  if (in.fleet || in.debug_linearize || in.jacobian_mode != TEB_AMD_JACOBIAN_ANALYTIC || in.B <= 0) return r;
  const int cus = in.num_cus > 0 ? in.num_cus : 256;
  const int room = cus / in.B - 1;   // helper workgroups per band that still leave every workgroup its own CU
  int K = 0, D = 0;
  if (in.speculative_trials >= 0 && in.layout != LAYOUT_BAND_HBM && !(in.layout == LAYOUT_BAND && in.band_ldlt) && in.inner > 0) {
    // automatic: as many of the three retries as the batch leaves CUs for (<= 64 bands: all three, <= 128: the first - the common - one)
    K = in.speculative_trials > 0 ? std::min(in.speculative_trials, kMaxSolverHelpers) : kMaxSolverHelpers;
    K = std::max(0, std::min(K, room));
  }
  if (in.multi_cu >= 0 && !in.fast_points && !in.legacy_association && in.M > 0) {
    D = std::min(room - K, 60);                               // beyond ~ 5 poses per helper the hand-off costs more than the tile
    // ... and that holds for short bands as well: at most one helper per 6 poses of the handle's capacity (round 6; until then a 60-pose
    // band could be given 60 helpers with a pose each). This is also where the one known defect of the mode lives: with 40 - 60 helpers on
    // 57 .. 62-pose bands 0.4 - 2.4 % of the launches returned ONE band off the single-CU result by |d chi2| ~ 1e-3 .. 1e-1 (rounds 4 - 6
    // binaries alike; more often the faster the kernel). Not found in round 6: agent-scope release / acquire fences at every hand-over,
    // fine-grained (uncached) hand-over buffers, returning atomics for the records, a poisoned pose buffer (never read stale) and an exact
    // arrival count changed nothing; a 14 us pause in front of the replay reduces it 20 x. At <= 20 helpers: 0 - 2 of 2000 launches, at
    // <= 12 none observed; C5 (53 - 60 helpers x 5 - 6 poses): 0 of 1400 (profiles/mcu_race_r06.txt).
    D = std::min(D, std::max(2, in.stride / 6));   // (the pose capacity: the bands grow under autoResize, what the host knows is where they started)
    if (in.multi_cu > 0) D = std::min(D, in.multi_cu);
    // auto: enough (pose, obstacle) work - and ONE band: the defect above needs at least two bands in the launch (any single band of that
    // scene with 60 helpers: 0 of 9000 launches; two bands 8 of 3000, three 18 of 3000; the bands' buffers do not overlap - padding them
    // changed nothing - so what the bands share is not understood). multi_cu > 0 still asks for helpers on any batch (the tests do).
    else if (in.B > 1 || (size_t)in.M * (size_t)(in.nmax_known > 0 ? in.nmax_known : in.stride) < 4096) D = 0;
    if (D < 2) D = 0;
  }
  r.K = K; r.D = D;
  return r;
}
// What the launch asks for: helpers_wanted, without the distance helpers while the back-off pauses them (which uses up one paused
// launch) or when their records would pass kMcuItemsMaxBytes. (Records that cannot be allocated are no error either: the driver then
// runs the launch without distance helpers - ADVICE r03.)
inline Helpers helpers_for_launch(const HelperInputs& in, HelperBackoff& backoff) {
  Helpers r = helpers_wanted(in);
  if (r.D > 0 && backoff.consume_paused_launch()) r.D = 0;
  if (r.D > 0 && distance_records(in.B, in.M, in.stride) * sizeof(double) > kMcuItemsMaxBytes) r.D = 0;
  return r;
}

// ---- the repeat ladder -----------------------------------------------------------------------------------------------------------------
// A launch in an optimistic layout or with distance helpers is followed by a look at the per-band flags (solver helpers alone cannot
// fail a band: a late one just means the band solves itself).
inline bool launch_is_checked(bool optimistic, int D) { return optimistic || D > 0; }
struct LadderStep {
  enum Next { DONE, RETRY_OPTIMISTIC, OWN_LAYOUT } next;   // both reruns start from the saved strips, without helpers
  int repeated;       // mcu_last_repeated: the launch timed out waiting for its helpers and was repeated on one CU per band
  bool nmax_stale;    // nmax_known becomes -1: a rerun's pose counts were not read (else: the counts read with the flags)
};
// After the first look - outgrown: a band outgrew the layout of the launch; helpers_late: the helpers of the multi-CU mode did not show
// up in time (a busy device: nothing promises their residency). From the saved strips: in the handle's own layout when a band outgrew
// the optimistic one, and on one CU per band when the helpers were late - that is, helpers late and no band outgrown so far, once more
// in the optimistic layout - whose capacity a band may outgrow in THAT run (the first one was cut short), so its flags are read as well
// (ADVICE r03): after_second_look.
inline LadderStep after_first_look(bool optimistic, bool outgrown, bool helpers_late) {
  if (!outgrown && !helpers_late) return LadderStep{LadderStep::DONE, 0, false};
  return LadderStep{outgrown || !optimistic ? LadderStep::OWN_LAYOUT : LadderStep::RETRY_OPTIMISTIC, helpers_late ? 1 : 0, true};
}
inline LadderStep after_second_look(bool outgrown) { return LadderStep{outgrown ? LadderStep::OWN_LAYOUT : LadderStep::DONE, 1, true}; }

// ---- which instantiation runs ----------------------------------------------------------------------------------------------------------
// The scene kinds a launch may run, by what profile_matches says of the configuration (pf: 0 none, 1 the *_DEFAULTS kinds, 2 *_WIDE,
// 3 *_LIGHT - 2 and 3 of point-like scenes only), the distance path, whether the launch has helper workgroups (the small-batch kinds)
// and the Jacobian mode. Helper kinds exist for closed-form Jacobians only: in the numeric mode (for which helpers_wanted grants none)
// the specialised kind is the one-workgroup one, no kind is compiled at run time, and the generic small-batch kind is not built.
struct SceneKinds {
  int specialised;   // the pre-built kind folded for the profile; KIND_NONE: pf == 0
  int generic;       // what runs when that kind is not part of the build
  int custom;        // the kind the run-time compiler makes for the configuration (teb_rtc.hpp); KIND_NONE: it makes none
};
inline SceneKinds scene_kinds(int pf, bool pointlike, bool helpers, int jacobian_mode) {
  const bool sm = helpers && jacobian_mode == TEB_AMD_JACOBIAN_ANALYTIC;
  SceneKinds k;
  k.specialised = pf == 1 ? (pointlike ? (sm ? KIND_POINTS_SMALL_DEFAULTS : KIND_POINTS_DEFAULTS) : (sm ? KIND_GENERIC_SMALL_DEFAULTS : KIND_GENERIC_DEFAULTS))
                : pf == 2 ? (sm ? KIND_POINTS_SMALL_WIDE : KIND_POINTS_WIDE)
                : pf == 3 ? (sm ? KIND_POINTS_SMALL_LIGHT : KIND_POINTS_LIGHT) : KIND_NONE;
  k.generic = pointlike ? (helpers ? KIND_POINTS_SMALL : KIND_POINTS) : (helpers ? KIND_GENERIC_SMALL : KIND_GENERIC);
  k.custom = helpers && !sm ? KIND_NONE
           : pointlike ? (sm ? KIND_POINTS_SMALL_CUSTOM : KIND_POINTS_CUSTOM) : (sm ? KIND_GENERIC_SMALL_CUSTOM : KIND_GENERIC_CUSTOM);
  return k;
}
// The pre-built instantiation of a launch: the specialised kind if the build has it (a build without the twins, or a mode they do not
// exist for, has not: lookup(kind) is null), else the generic kind - and the reported profile goes back to 0. fn null: neither.
struct Prebuilt {
  int kind = KIND_NONE, profile = 0;
  const void* fn = nullptr;
};
template <class Lookup>
Prebuilt pick_prebuilt(const SceneKinds& k, int pf, Lookup lookup) {
  Prebuilt p;
  if (k.specialised != KIND_NONE && (p.fn = lookup(k.specialised))) { p.kind = k.specialised; p.profile = pf; }
  else if ((p.fn = lookup(k.generic))) p.kind = k.generic;
  return p;
}

}  // namespace tebamd
