// launch_host_check.cpp — csrc/teb_launch_host.hpp on its own (no HIP): the policy of the optimise launch against answers written out by
// hand. Stand-alone: tests/test_launch_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; it prints
// what failed and returns the number of failures.
//
// The LDS plan is synthetic, so that every threshold can be worked out in a comment:
//   bytes(S, layout, cache) = per_pose[layout] * S + 8 * cache, per_pose = 100 (blocks), 50 (LDS band), 10 (band in HBM)
// Against a limit of 20000 B and without a cache the blocks hold 200 poses, the LDS band 400, the band in HBM 2000.
#include "../../teb_local_planner_amd/csrc/teb_launch_host.hpp"

#include <cstdio>

using namespace tebamd;

static int g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

static size_t plan_bytes(int S, int layout, int cache) {
  const int per_pose = layout == LAYOUT_BLOCKS ? 100 : layout == LAYOUT_BAND ? 50 : 10;
  return (size_t)per_pose * S + (size_t)8 * cache;
}
static const size_t kLimit = 20000;
static const int kLanes = 256, kIterHbm = 4;   // two poses per lane in the LDS layouts (512), four with the band in HBM (1024)

static CreateLayout create(int max_poses, int max_obstacles, int pin, size_t limit = kLimit) {
  return layout_at_create(max_poses, max_obstacles, limit, pin, kLanes, kIterHbm, plan_bytes);
}
static bool made(const CreateLayout& r, int layout) { return r.refused == CreateLayout::NO && r.layout == layout; }

static void check_create() {
  // automatic, no obstacles: blocks to 200 poses, the LDS band to 400, the band in HBM beyond
  CHECK(made(create(200, 0, TEB_AMD_LAYOUT_AUTO), LAYOUT_BLOCKS));
  CHECK(made(create(201, 0, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND));
  CHECK(made(create(400, 0, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND));
  CHECK(made(create(401, 0, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND_HBM));   // 50 * 401 = 20050 > 20000
  CHECK(made(create(200, -3, TEB_AMD_LAYOUT_AUTO), LAYOUT_BLOCKS));    // (a negative obstacle capacity counts as none)
  // 150 poses with the cache of a full table: the blocks take 15000 + 8 M <= 20000 up to M = 625; beyond, the band (7500 + 8 M) if IT
  // holds the cache, up to M = 1562 - else the blocks stay (and the table will run without the cache)
  CHECK(made(create(150, 625, TEB_AMD_LAYOUT_AUTO), LAYOUT_BLOCKS));
  CHECK(made(create(150, 626, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND));
  CHECK(made(create(150, 1562, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND));
  CHECK(made(create(150, 1563, TEB_AMD_LAYOUT_AUTO), LAYOUT_BLOCKS));
  // every pin
  CHECK(made(create(100, 0, TEB_AMD_LAYOUT_BAND_LDS), LAYOUT_BAND));
  CHECK(made(create(100, 0, TEB_AMD_LAYOUT_BAND_HBM), LAYOUT_BAND_HBM));
  CHECK(made(create(200, 2000, TEB_AMD_LAYOUT_BLOCKS_LDS), LAYOUT_BLOCKS));   // (the cache does not move a pinned layout)
  CHECK(create(201, 0, TEB_AMD_LAYOUT_BLOCKS_LDS).refused == CreateLayout::BLOCKS_TOO_LARGE);
  CHECK(made(create(400, 0, TEB_AMD_LAYOUT_BAND_LDS), LAYOUT_BAND));
  CHECK(made(create(401, 0, TEB_AMD_LAYOUT_BAND_LDS), LAYOUT_BAND_HBM));      // a pinned LDS band too long for the LDS moves all the same
  // one pose above two per lane: with 30000 B the LDS band would hold 600 poses, its instantiations hold 512
  CHECK(made(create(512, 0, TEB_AMD_LAYOUT_AUTO, 30000), LAYOUT_BAND));
  CHECK(made(create(513, 0, TEB_AMD_LAYOUT_AUTO, 30000), LAYOUT_BAND_HBM));
  CHECK(made(create(513, 0, TEB_AMD_LAYOUT_BAND_LDS, 30000), LAYOUT_BAND_HBM));
  // the capacity refusal, by lanes (1024 poses of the band in HBM) ..
  CHECK(made(create(1024, 0, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND_HBM));
  const CreateLayout lanes = create(1025, 0, TEB_AMD_LAYOUT_AUTO);
  CHECK(lanes.refused == CreateLayout::CAPACITY && lanes.layout == LAYOUT_BAND_HBM && lanes.thread_limit == 1024 && lanes.lds == 10250);
  // .. and by LDS: 5000 B hold 500 poses of the band in HBM
  CHECK(made(create(500, 0, TEB_AMD_LAYOUT_AUTO, 5000), LAYOUT_BAND_HBM));
  const CreateLayout lds = create(501, 0, TEB_AMD_LAYOUT_AUTO, 5000);
  CHECK(lds.refused == CreateLayout::CAPACITY && lds.lds == 5010 && lds.thread_limit == 1024);
  CHECK(made(create(1024, 0, TEB_AMD_LAYOUT_AUTO), LAYOUT_BAND_HBM) && create(1024, 0, TEB_AMD_LAYOUT_AUTO).thread_limit == 1024);
  CHECK(create(100, 0, TEB_AMD_LAYOUT_AUTO).thread_limit == 512);
}

static TableLayout table(bool rows, int footprint, bool generic_path, int created, int pin, int M, int stride) {
  return layout_per_table(rows, footprint, generic_path, created, pin, M, stride, kLimit, plan_bytes);
}
static bool is(const TableLayout& t, int layout, int fast, int cache, bool hbm) {
  return t.layout == layout && t.fast_points == fast && t.cache_entries == cache && t.hbm_band == hbm;
}

static void check_table() {
  const int P = TEB_AMD_FOOTPRINT_POINT, A = TEB_AMD_LAYOUT_AUTO;
  // an LDS band handle of 300 poses (15000 B): the cache fits up to 625 entries; one more and the band moves to HBM (3000 + 8 M),
  // which keeps the cache up to M = 2125; beyond, the band stays where it was and the table runs on the generic path
  CHECK(is(table(true, P, false, LAYOUT_BAND, A, 625, 300), LAYOUT_BAND, 1, 625, false));
  CHECK(is(table(true, P, false, LAYOUT_BAND, A, 626, 300), LAYOUT_BAND_HBM, 1, 626, true));
  CHECK(is(table(true, P, false, LAYOUT_BAND, A, 2125, 300), LAYOUT_BAND_HBM, 1, 2125, true));
  CHECK(is(table(true, P, false, LAYOUT_BAND, A, 2126, 300), LAYOUT_BAND, 0, 0, false));
  CHECK(is(table(true, P, false, LAYOUT_BAND, TEB_AMD_LAYOUT_BAND_LDS, 626, 300), LAYOUT_BAND, 0, 0, false));   // a pinned band does not move
  // a block handle of 150 poses (15000 B): one entry too many and the cache is gone, the layout stays
  CHECK(is(table(true, P, false, LAYOUT_BLOCKS, A, 625, 150), LAYOUT_BLOCKS, 1, 625, false));
  CHECK(is(table(true, P, false, LAYOUT_BLOCKS, A, 626, 150), LAYOUT_BLOCKS, 0, 0, false));
  // a handle with the band in HBM already (400 poses: 4000 B) needs nothing new
  CHECK(is(table(true, P, false, LAYOUT_BAND_HBM, A, 2000, 400), LAYOUT_BAND_HBM, 1, 2000, false));
  CHECK(is(table(true, P, false, LAYOUT_BAND_HBM, A, 2001, 400), LAYOUT_BAND_HBM, 0, 0, false));
  // what makes a table generic: its rows, the footprint, the switch, no rows at all
  CHECK(is(table(true, TEB_AMD_FOOTPRINT_CIRCULAR, false, LAYOUT_BAND, A, 10, 300), LAYOUT_BAND, 1, 10, false));
  CHECK(is(table(false, P, false, LAYOUT_BAND, A, 10, 300), LAYOUT_BAND, 0, 0, false));
  CHECK(is(table(true, TEB_AMD_FOOTPRINT_POLYGON, false, LAYOUT_BAND, A, 10, 300), LAYOUT_BAND, 0, 0, false));
  CHECK(is(table(true, TEB_AMD_FOOTPRINT_TWO_CIRCLES, false, LAYOUT_BAND, A, 10, 300), LAYOUT_BAND, 0, 0, false));
  CHECK(is(table(true, TEB_AMD_FOOTPRINT_LINE, false, LAYOUT_BAND, A, 626, 300), LAYOUT_BAND, 0, 0, false));   // (and no move for a cache that is not used)
  CHECK(is(table(true, P, true, LAYOUT_BAND, A, 10, 300), LAYOUT_BAND, 0, 0, false));
  CHECK(is(table(true, P, true, LAYOUT_BAND, A, 626, 300), LAYOUT_BAND, 0, 0, false));
  CHECK(is(table(true, P, false, LAYOUT_BAND, A, 0, 300), LAYOUT_BAND, 0, 0, false));
}

static const LayoutSwitches kNoSwitch{false, false, false, false};
static LaunchLayout per_launch(int own, const LayoutSwitches& sw, int nmax, int stride, int cache) {
  return layout_per_launch(own, sw, nmax, stride, cache, kLimit, plan_bytes);
}
static bool is(const LaunchLayout& l, int layout, int S, bool optimistic) { return l.layout == layout && l.S == S && l.optimistic == optimistic; }

static void check_launch_layout() {
  // the capacity search: downwards from `upto`, not below 8 poses
  CHECK(max_capacity_of(LAYOUT_BLOCKS, 238, 0, kLimit, plan_bytes) == 200);
  CHECK(max_capacity_of(LAYOUT_BLOCKS, 150, 0, kLimit, plan_bytes) == 150);
  CHECK(max_capacity_of(LAYOUT_BAND, 337, 0, kLimit, plan_bytes) == 337);
  CHECK(max_capacity_of(LAYOUT_BLOCKS, 238, 2400, kLimit, plan_bytes) == 8);    // 800 + 19200 = 20000
  CHECK(max_capacity_of(LAYOUT_BLOCKS, 238, 2401, kLimit, plan_bytes) == 0);    // 800 + 19208: nothing fits
  CHECK(max_capacity_of(LAYOUT_BLOCKS, 5, 0, kLimit, plan_bytes) == 5);
  CHECK(max_capacity_of(LAYOUT_BLOCKS, 5, 2500, kLimit, plan_bytes) == 0);
  // a handle with the band in HBM, 400 poses, no cache: blocks hold s = 200. need = nmax + nmax / 10 + 4: 179 -> 200, 180 -> 202
  CHECK(is(per_launch(LAYOUT_BAND_HBM, kNoSwitch, 179, 400, 0), LAYOUT_BLOCKS, 200, true));
  CHECK(is(per_launch(LAYOUT_BAND_HBM, kNoSwitch, 180, 400, 0), LAYOUT_BAND, 337, true));     // the band rung: 50 * 337 fits
  // with a cache of 13 entries (104 B) the blocks hold 198: nmax 177 -> need 198 = s, 178 -> 199 = s + 1
  CHECK(is(per_launch(LAYOUT_BAND_HBM, kNoSwitch, 177, 400, 13), LAYOUT_BLOCKS, 198, true));
  CHECK(is(per_launch(LAYOUT_BAND_HBM, kNoSwitch, 178, 400, 13), LAYOUT_BAND, 337, true));
  // the band rung holds 337: nmax 303 -> need 337, 304 -> 338: the handle's own layout, its own plan
  CHECK(is(per_launch(LAYOUT_BAND_HBM, kNoSwitch, 303, 400, 0), LAYOUT_BAND, 337, true));
  CHECK(is(per_launch(LAYOUT_BAND_HBM, kNoSwitch, 304, 400, 0), LAYOUT_BAND_HBM, 400, false));
  // an LDS band handle has the block rung only
  CHECK(is(per_launch(LAYOUT_BAND, kNoSwitch, 179, 300, 0), LAYOUT_BLOCKS, 200, true));
  CHECK(is(per_launch(LAYOUT_BAND, kNoSwitch, 180, 300, 0), LAYOUT_BAND, 300, false));
  // a short handle that is a band for its cache's sake (150 poses, 626 entries: blocks hold 149): the capacity ends at the stride
  CHECK(is(per_launch(LAYOUT_BAND, kNoSwitch, 132, 150, 626), LAYOUT_BLOCKS, 149, true));     // 132 + 13 + 4 = 149
  CHECK(is(per_launch(LAYOUT_BAND, kNoSwitch, 133, 150, 626), LAYOUT_BAND, 150, false));
  CHECK(is(per_launch(LAYOUT_BAND, kNoSwitch, 0, 150, 2401), LAYOUT_BAND, 150, false));       // no capacity at all
  // a block handle is where it wants to be; each of the four switches keeps the own layout
  CHECK(!may_launch_optimistic(LAYOUT_BLOCKS, kNoSwitch) && may_launch_optimistic(LAYOUT_BAND, kNoSwitch) && may_launch_optimistic(LAYOUT_BAND_HBM, kNoSwitch));
  CHECK(is(per_launch(LAYOUT_BLOCKS, kNoSwitch, 20, 200, 0), LAYOUT_BLOCKS, 200, false));
  const LayoutSwitches each[4] = {{true, false, false, false}, {false, true, false, false}, {false, false, true, false}, {false, false, false, true}};
  for (const LayoutSwitches& sw : each) {
    CHECK(!may_launch_optimistic(LAYOUT_BAND_HBM, sw));
    CHECK(is(per_launch(LAYOUT_BAND_HBM, sw, 20, 400, 0), LAYOUT_BAND_HBM, 400, false));
  }
}

// one band of 50 poses (capacity 60) against 100 generic obstacles on 256 CUs, everything automatic, blocks in LDS, 5 inner iterations
static HelperInputs base_inputs() {
  HelperInputs in;
  in.fleet = false; in.debug_linearize = false; in.jacobian_mode = TEB_AMD_JACOBIAN_ANALYTIC;
  in.B = 1; in.M = 100; in.stride = 60; in.nmax_known = 50; in.num_cus = 256;
  in.speculative_trials = 0; in.multi_cu = 0; in.layout = LAYOUT_BLOCKS; in.band_ldlt = false; in.inner = 5;
  in.fast_points = false; in.legacy_association = false;
  return in;
}
static bool is(const Helpers& h, int K, int D) { return h.K == K && h.D == D; }

static void check_helpers() {
  // the base: room 255, K = 3, D = min(252, 60) -> one per 6 poses of the capacity: 10; 100 * 50 = 5000 >= 4096
  CHECK(is(helpers_wanted(base_inputs()), 3, 10));
  {   // the room cus / B - 1 at 256 CUs. multi_cu = 60 asks for distance helpers on any batch
    const int Bs[7] = {1, 64, 65, 128, 129, 256, 300}, K[7] = {3, 3, 2, 1, 0, 0, 0}, D[7] = {10, 0, 0, 0, 0, 0, 0};   // room 255, 3, 2, 1, 0, 0, -1
    for (int i = 0; i < 7; ++i) {
      HelperInputs in = base_inputs();
      in.B = Bs[i]; in.multi_cu = 60;
      CHECK(is(helpers_wanted(in), K[i], D[i]));
    }
    HelperInputs in = base_inputs();
    in.num_cus = 0;    // unknown: 256
    CHECK(is(helpers_wanted(in), 3, 10));
    in.num_cus = 8;    // room 7: K = 3, D = 4
    CHECK(is(helpers_wanted(in), 3, 4));
    in.num_cus = 5;    // room 4: K = 3, D = 1 -> 0
    CHECK(is(helpers_wanted(in), 3, 0));
    in.B = 0;
    CHECK(is(helpers_wanted(in), 0, 0));
  }
  {   // K by speculative_trials, and the layouts without solver helpers
    const int st[4] = {-1, 0, 2, 9}, K[4] = {0, 3, 2, 3}, D[4] = {10, 10, 10, 10};
    for (int i = 0; i < 4; ++i) {
      HelperInputs in = base_inputs();
      in.speculative_trials = st[i];
      CHECK(is(helpers_wanted(in), K[i], D[i]));
    }
    HelperInputs in = base_inputs();
    in.layout = LAYOUT_BAND_HBM;
    CHECK(is(helpers_wanted(in), 0, 10));
    in.layout = LAYOUT_BAND;
    CHECK(is(helpers_wanted(in), 3, 10));
    in.band_ldlt = true;
    CHECK(is(helpers_wanted(in), 0, 10));
    in.layout = LAYOUT_BLOCKS;   // (the switch means the LDS band only)
    CHECK(is(helpers_wanted(in), 3, 10));
    in.inner = 0;
    CHECK(is(helpers_wanted(in), 0, 10));
  }
  {   // D: automatic against multi_cu > 0; the guard of the multi-band defect (B > 1 in auto: none)
    HelperInputs in = base_inputs();
    in.B = 3;                    // room 84, K = 3
    CHECK(is(helpers_wanted(in), 3, 0));
    in.multi_cu = 4;             // min(81, 60) -> 10 -> 4
    CHECK(is(helpers_wanted(in), 3, 4));
    in.multi_cu = 60;
    CHECK(is(helpers_wanted(in), 3, 10));
    in.multi_cu = 1;             // one helper is none
    CHECK(is(helpers_wanted(in), 3, 0));
    in.multi_cu = -1;            // off
    CHECK(is(helpers_wanted(in), 3, 0));
    in.B = 1;
    CHECK(is(helpers_wanted(in), 3, 0));
    in.multi_cu = 2;
    CHECK(is(helpers_wanted(in), 3, 2));
  }
  {   // auto: M * n >= 4096, n the longest band if the host knows it, else the capacity
    HelperInputs in = base_inputs();
    in.M = 91; in.nmax_known = 45; in.stride = 64;    // 4095
    CHECK(is(helpers_wanted(in), 3, 0));
    in.M = 64; in.nmax_known = 64;                    // 4096; 64 / 6 = 10
    CHECK(is(helpers_wanted(in), 3, 10));
    in.M = 100; in.nmax_known = -1; in.stride = 40;   // 4000
    CHECK(is(helpers_wanted(in), 3, 0));
    in.stride = 41;                                   // 4100; 41 / 6 = 6
    CHECK(is(helpers_wanted(in), 3, 6));
    in.nmax_known = 0; in.stride = 40;
    CHECK(is(helpers_wanted(in), 3, 0));
    in.multi_cu = 60;                                 // asked for: no threshold
    CHECK(is(helpers_wanted(in), 3, 6));
  }
  {   // at most one distance helper per 6 poses of the capacity, at least 2, at most 60
    const int stride[4] = {11, 12, 60, 400}, D[4] = {2, 2, 10, 60};
    for (int i = 0; i < 4; ++i) {
      HelperInputs in = base_inputs();
      in.multi_cu = 100; in.stride = stride[i];
      CHECK(is(helpers_wanted(in), 3, D[i]));
    }
  }
  {   // no helpers at all: numeric Jacobians, the debug launch, a fleet; no distance helpers: legacy association, a point-like scene, no obstacles
    HelperInputs in = base_inputs();
    in.jacobian_mode = TEB_AMD_JACOBIAN_G2O_NUMERIC;
    CHECK(is(helpers_wanted(in), 0, 0));
    in = base_inputs(); in.debug_linearize = true;
    CHECK(is(helpers_wanted(in), 0, 0));
    in = base_inputs(); in.fleet = true; in.multi_cu = 60;
    CHECK(is(helpers_wanted(in), 0, 0));
    in = base_inputs(); in.legacy_association = true;
    CHECK(is(helpers_wanted(in), 3, 0));
    in = base_inputs(); in.fast_points = true;
    CHECK(is(helpers_wanted(in), 3, 0));
    in = base_inputs(); in.M = 0; in.multi_cu = 60;
    CHECK(is(helpers_wanted(in), 3, 0));
  }
  {   // the pause uses up a launch - one that would have had distance helpers, no other
    HelperBackoff bo;
    bo.left = 2; bo.len = 4;
    CHECK(is(helpers_for_launch(base_inputs(), bo), 3, 0) && bo.left == 1 && bo.len == 4);
    HelperInputs points = base_inputs();
    points.fast_points = true;
    CHECK(is(helpers_for_launch(points, bo), 3, 0) && bo.left == 1);
    CHECK(is(helpers_for_launch(base_inputs(), bo), 3, 0) && bo.left == 0);
    CHECK(is(helpers_for_launch(base_inputs(), bo), 3, 10) && bo.left == 0 && bo.len == 4);   // the probe
  }
  {   // distance records [B][M][4][stride] doubles: 65536 obstacles x 512 poses are exactly 1 GiB; one obstacle more is beyond
    HelperBackoff bo;
    HelperInputs in = base_inputs();
    in.M = 65536; in.stride = 512; in.multi_cu = 8;
    CHECK(distance_records(in.B, in.M, in.stride) * sizeof(double) == kMcuItemsMaxBytes);
    CHECK(is(helpers_for_launch(in, bo), 3, 8));
    in.M = 65537;
    CHECK(is(helpers_wanted(in), 3, 8) && is(helpers_for_launch(in, bo), 3, 0));
    in.M = 32768; in.B = 2;                                      // 1 GiB again
    CHECK(is(helpers_for_launch(in, bo), 3, 8));
    in.B = 3;
    CHECK(is(helpers_for_launch(in, bo), 3, 0));
    bo.left = 1; bo.len = 4;                                     // (too large AND paused: the pause is used up first)
    CHECK(is(helpers_for_launch(in, bo), 3, 0) && bo.left == 0);
  }
}

static void check_backoff() {
  HelperBackoff bo;
  CHECK(!bo.consume_paused_launch() && bo.left == 0);
  const int len[9] = {4, 8, 16, 32, 64, 128, 256, 256, 256};
  for (int i = 0; i < 9; ++i) {
    bo.update(true);
    CHECK(bo.len == len[i] && bo.left == len[i]);
  }
  CHECK(bo.consume_paused_launch() && bo.left == 255 && bo.len == 256);
  bo.update(false);   // a good probe
  CHECK(bo.len == 0 && bo.left == 0 && !bo.consume_paused_launch());
  bo.update(false);
  CHECK(bo.len == 0 && bo.left == 0);
  bo.update(true);
  CHECK(bo.len == 4 && bo.consume_paused_launch() && bo.consume_paused_launch() && bo.consume_paused_launch() && bo.consume_paused_launch() &&
        !bo.consume_paused_launch() && bo.left == 0 && bo.len == 4);
  // the wait for helpers: 100 ticks per us, 2 ms unless set; 250 us at most while a pause is remembered
  CHECK(helper_timeout_ticks(0) == 200000 && helper_timeout_ticks(-5) == 200000 && helper_timeout_ticks(500) == 50000);
  CHECK(bo.probe_timeout(200000) == 25000 && bo.probe_timeout(25000) == 25000 && bo.probe_timeout(10000) == 10000);
  bo.update(false);
  CHECK(bo.probe_timeout(200000) == 200000);
}

static bool is(const LadderStep& s, LadderStep::Next next, int repeated, bool stale) { return s.next == next && s.repeated == repeated && s.nmax_stale == stale; }

static void check_ladder() {
  CHECK(!launch_is_checked(false, 0) && launch_is_checked(true, 0) && launch_is_checked(false, 2) && launch_is_checked(true, 2));
  // (optimistic, outgrown, helpers late)
  CHECK(is(after_first_look(false, false, false), LadderStep::DONE, 0, false));
  CHECK(is(after_first_look(true, false, false), LadderStep::DONE, 0, false));
  CHECK(is(after_first_look(false, true, false), LadderStep::OWN_LAYOUT, 0, true));
  CHECK(is(after_first_look(true, true, false), LadderStep::OWN_LAYOUT, 0, true));
  CHECK(is(after_first_look(false, false, true), LadderStep::OWN_LAYOUT, 1, true));         // the own layout IS the layout of the launch: once more without helpers
  CHECK(is(after_first_look(true, false, true), LadderStep::RETRY_OPTIMISTIC, 1, true));
  CHECK(is(after_first_look(false, true, true), LadderStep::OWN_LAYOUT, 1, true));
  CHECK(is(after_first_look(true, true, true), LadderStep::OWN_LAYOUT, 1, true));
  // the second look follows RETRY_OPTIMISTIC only: the launch was repeated for its helpers either way
  CHECK(is(after_second_look(false), LadderStep::DONE, 1, true));
  CHECK(is(after_second_look(true), LadderStep::OWN_LAYOUT, 1, true));
}

static void check_kinds() {
  const int A = TEB_AMD_JACOBIAN_ANALYTIC, N = TEB_AMD_JACOBIAN_G2O_NUMERIC, X = KIND_NONE;
  // [pf][point-like][helpers][Jacobian mode] -> specialised, generic, custom
  struct Row { int pf; bool points, helpers; int jm, specialised, generic, custom; };
  const Row rows[32] = {
      {0, false, false, A, X, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {0, false, false, N, X, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {0, false, true, A, X, KIND_GENERIC_SMALL, KIND_GENERIC_SMALL_CUSTOM},
      {0, false, true, N, X, KIND_GENERIC_SMALL, X},
      {0, true, false, A, X, KIND_POINTS, KIND_POINTS_CUSTOM},
      {0, true, false, N, X, KIND_POINTS, KIND_POINTS_CUSTOM},
      {0, true, true, A, X, KIND_POINTS_SMALL, KIND_POINTS_SMALL_CUSTOM},
      {0, true, true, N, X, KIND_POINTS_SMALL, X},
      {1, false, false, A, KIND_GENERIC_DEFAULTS, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {1, false, false, N, KIND_GENERIC_DEFAULTS, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {1, false, true, A, KIND_GENERIC_SMALL_DEFAULTS, KIND_GENERIC_SMALL, KIND_GENERIC_SMALL_CUSTOM},
      {1, false, true, N, KIND_GENERIC_DEFAULTS, KIND_GENERIC_SMALL, X},
      {1, true, false, A, KIND_POINTS_DEFAULTS, KIND_POINTS, KIND_POINTS_CUSTOM},
      {1, true, false, N, KIND_POINTS_DEFAULTS, KIND_POINTS, KIND_POINTS_CUSTOM},
      {1, true, true, A, KIND_POINTS_SMALL_DEFAULTS, KIND_POINTS_SMALL, KIND_POINTS_SMALL_CUSTOM},
      {1, true, true, N, KIND_POINTS_DEFAULTS, KIND_POINTS_SMALL, X},
      // (profile_matches answers 2 and 3 for point-like scenes only; the *_WIDE and *_LIGHT kinds are point-like whatever is asked)
      {2, false, false, A, KIND_POINTS_WIDE, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {2, false, false, N, KIND_POINTS_WIDE, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {2, false, true, A, KIND_POINTS_SMALL_WIDE, KIND_GENERIC_SMALL, KIND_GENERIC_SMALL_CUSTOM},
      {2, false, true, N, KIND_POINTS_WIDE, KIND_GENERIC_SMALL, X},
      {2, true, false, A, KIND_POINTS_WIDE, KIND_POINTS, KIND_POINTS_CUSTOM},
      {2, true, false, N, KIND_POINTS_WIDE, KIND_POINTS, KIND_POINTS_CUSTOM},
      {2, true, true, A, KIND_POINTS_SMALL_WIDE, KIND_POINTS_SMALL, KIND_POINTS_SMALL_CUSTOM},
      {2, true, true, N, KIND_POINTS_WIDE, KIND_POINTS_SMALL, X},
      {3, false, false, A, KIND_POINTS_LIGHT, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {3, false, false, N, KIND_POINTS_LIGHT, KIND_GENERIC, KIND_GENERIC_CUSTOM},
      {3, false, true, A, KIND_POINTS_SMALL_LIGHT, KIND_GENERIC_SMALL, KIND_GENERIC_SMALL_CUSTOM},
      {3, false, true, N, KIND_POINTS_LIGHT, KIND_GENERIC_SMALL, X},
      {3, true, false, A, KIND_POINTS_LIGHT, KIND_POINTS, KIND_POINTS_CUSTOM},
      {3, true, false, N, KIND_POINTS_LIGHT, KIND_POINTS, KIND_POINTS_CUSTOM},
      {3, true, true, A, KIND_POINTS_SMALL_LIGHT, KIND_POINTS_SMALL, KIND_POINTS_SMALL_CUSTOM},
      {3, true, true, N, KIND_POINTS_LIGHT, KIND_POINTS_SMALL, X},
  };
  unsigned seen = 0;
  for (const Row& r : rows) {
    const SceneKinds k = scene_kinds(r.pf, r.points, r.helpers, r.jm);
    if (!(k.specialised == r.specialised && k.generic == r.generic && k.custom == r.custom)) {
      std::printf("FAILED scene_kinds(%d, %d, %d, %d) = %d, %d, %d\n", r.pf, (int)r.points, (int)r.helpers, r.jm, k.specialised, k.generic, k.custom);
      ++g_failures;
    }
    seen |= 1u << (r.pf * 8 + r.points * 4 + r.helpers * 2 + r.jm);
  }
  CHECK(seen == 0xffffffffu);   // all 32 cells
  // the pre-built pick: a build that has every kind, one without the specialised twins, one with nothing
  static const char kFn[16] = {};
  const auto all = [](int kind) -> const void* { return kind >= 0 && kind < 12 ? &kFn[kind] : nullptr; };
  const auto plain = [](int kind) -> const void* { return kind >= 0 && kind < 4 ? &kFn[kind] : nullptr; };
  const auto nothing = [](int) -> const void* { return nullptr; };
  const SceneKinds wide = scene_kinds(2, true, false, A);
  Prebuilt p = pick_prebuilt(wide, 2, all);
  CHECK(p.kind == KIND_POINTS_WIDE && p.profile == 2 && p.fn == &kFn[KIND_POINTS_WIDE]);
  p = pick_prebuilt(wide, 2, plain);
  CHECK(p.kind == KIND_POINTS && p.profile == 0 && p.fn == &kFn[KIND_POINTS]);
  p = pick_prebuilt(wide, 2, nothing);
  CHECK(p.kind == KIND_NONE && p.profile == 0 && p.fn == nullptr);
  p = pick_prebuilt(scene_kinds(0, false, true, A), 0, all);
  CHECK(p.kind == KIND_GENERIC_SMALL && p.profile == 0 && p.fn == &kFn[KIND_GENERIC_SMALL]);
  p = pick_prebuilt(scene_kinds(1, false, true, A), 1, all);
  CHECK(p.kind == KIND_GENERIC_SMALL_DEFAULTS && p.profile == 1);
}

int main() {
  check_create();
  check_table();
  check_launch_layout();
  check_helpers();
  check_backoff();
  check_ladder();
  check_kinds();
  if (g_failures) {
    std::printf("%d check(s) failed\n", g_failures);
    return 1;
  }
  std::printf("launch host check ok\n");
  return 0;
}
