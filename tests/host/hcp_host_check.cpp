// hcp_host_check.cpp — csrc/teb_hcp_host.hpp on its own (no HIP): the host rules of one HomotopyClassPlanner against answers written
// out by hand from the reference's text (src/graph_search.cpp, src/homotopy_class_planner.cpp, h_signature.h). Stand-alone:
// tests/test_hcp_host.py compiles it with the address and undefined-behaviour sanitizers and runs it; it prints what failed and
// returns the number of failures. All coordinates and thresholds are binary fractions, so every expected value is exact.
#define TEB_SCENE_STORE_HOST_ONLY
#include "../../teb_local_planner_amd/csrc/teb_hcp_host.hpp"

#include <cstdio>
#include <cstring>

using namespace tebamd;

static int g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

typedef std::vector<int> Path;
typedef std::vector<std::vector<int>> Adj;

// vertices 0..3, edges 0->1, 0->2, 1->2, 1->3, 2->3 as the byte matrix of the edge kernel
static const unsigned char kDiamond[16] = {0, 1, 1, 0,  0, 0, 1, 1,  0, 0, 0, 1,  0, 0, 0, 0};

static void check_path_enumerator() {
  const Adj adj = adjacency_lists(kDiamond, 4);
  CHECK((adj == Adj{{1, 2}, {2, 3}, {3}, {}}));
  {   // DepthFirst: the goal, if adjacent, closes a path before the recursion into the other neighbours
    PathEnumerator en(adj, 0, 3);
    Path p;
    CHECK(en.next(p) && (p == Path{0, 1, 3}));
    CHECK(en.next(p) && (p == Path{0, 1, 2, 3}));
    CHECK(en.next(p) && (p == Path{0, 2, 3}));
    CHECK(!en.next(p));
    CHECK(!en.next(p));
  }
  {   // vertex 1 is a dead end: 0->1, 0->2, 2->3
    PathEnumerator en(Adj{{1, 2}, {}, {3}, {}}, 0, 3);
    Path p;
    CHECK(en.next(p) && (p == Path{0, 2, 3}));
    CHECK(!en.next(p));
  }
  {   // two expansions reach the first path (vertex 0, vertex 1); the third ends the enumeration
    PathEnumerator en(adj, 0, 3);
    en.max_expansions = 2;
    Path p;
    CHECK(en.next(p) && (p == Path{0, 1, 3}));
    CHECK(!en.next(p));
    PathEnumerator one(adj, 0, 3);
    one.max_expansions = 1;
    CHECK(!one.next(p));
  }
}

static void check_take_paths() {
  const std::vector<double> vx = {0, 10, 20, 30}, vy = {0, 1, 2, 3};
  {   // rounds of two
    PathSource ps(adjacency_lists(kDiamond, 4), 0);
    std::vector<double> px, py;
    std::vector<int> off(1, 0);
    CHECK(take_paths(ps, 2, 0, 5, vx, vy, px, py, off) == 2 && ps.more);
    CHECK((off == std::vector<int>{0, 3, 7}));
    CHECK((px == std::vector<double>{0, 10, 30, 0, 10, 20, 30}) && (py == std::vector<double>{0, 1, 3, 0, 1, 2, 3}));
    off.assign(1, 0); px.clear(); py.clear();
    CHECK(take_paths(ps, 2, 0, 5, vx, vy, px, py, off) == 1 && !ps.more);
    CHECK((px == std::vector<double>{0, 20, 30}));
  }
  {   // a budget of two examined paths ends the source with the round that reaches it
    PathSource ps(adjacency_lists(kDiamond, 4), 2);
    std::vector<double> px, py;
    std::vector<int> off(1, 0);
    CHECK(ps.en.max_expansions == 20000);
    CHECK(take_paths(ps, 64, 2, 5, vx, vy, px, py, off) == 2 && !ps.more);
    ps.examined = 2;
    CHECK(take_paths(ps, 64, 2, 5, vx, vy, px, py, off) == 0);
  }
  {   // the second path has four vertices
    PathSource ps(adjacency_lists(kDiamond, 4), 0);
    std::vector<double> px, py;
    std::vector<int> off(1, 0);
    CHECK(take_paths(ps, 1, 0, 3, vx, vy, px, py, off) == 1);
    CHECK(take_paths(ps, 1, 0, 3, vx, vy, px, py, off) == -1);
  }
}

static void check_predicates() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  SignatureRule r2;
  r2.mode = 2; r2.W = 2; r2.thr = 0.25;
  {   // HSignature::isEqual: |difference| <= threshold in both parts
    const double a[2] = {1, -1}, at[2] = {1.25, -1.25}, past[2] = {1.25, -1.5}, big[2] = {4, 0}, bad[2] = {0, inf}, worse[2] = {nan, 0};
    CHECK(r2.equal(a, at) && r2.equal(at, a));
    CHECK(!r2.equal(a, past) && !r2.equal(past, a));
    CHECK(r2.valid(a) && !r2.valid(bad) && !r2.valid(worse));
    CHECK(r2.reasonable(big));   // only HSignature3d values are bounded by 1
  }
  SignatureRule r3;
  r3.mode = 3; r3.W = 3; r3.thr = 0.25;
  {   // HSignature3d::isEqual: values below the threshold on either side are ignored; the others must agree in sign
    const double a[3] = {0.125, 0.5, -0.125}, b[3] = {-0.125, 0.75, 0.125}, c[3] = {-0.5, 0.5, 0.125}, d[3] = {0.125, -0.5, 0};
    const double at[3] = {0.25, 0.5, 0}, opp[3] = {-0.25, 0.5, 0}, big[3] = {0, 1.5, 0}, one[3] = {1, -3, 0}, bad[3] = {0, 0, -inf};
    CHECK(r3.equal(a, b) && r3.equal(b, a));
    CHECK(r3.equal(a, c));       // 0.125 against -0.5: the small side hides the pair
    CHECK(!r3.equal(a, d) && !r3.equal(d, a));   // 0.5 against -0.5
    CHECK(!r3.equal(at, opp));   // a value AT the threshold counts (the test is <)
    CHECK(r3.valid(a) && !r3.valid(bad));
    CHECK(r3.reasonable(a) && r3.reasonable(one) && !r3.reasonable(big));
  }
  SignatureRule r0;   // a planner without obstacles: empty rows are valid and equal
  r0.mode = 3; r0.W = 0;
  CHECK(r0.valid(nullptr) && r0.reasonable(nullptr) && r0.equal(nullptr, nullptr));
}

// class A three times (A, A1, A2 pairwise within the threshold), class B once, an invalid row
static const double kB[2] = {3, 0}, kA[2] = {1, 0}, kA1[2] = {1.125, 0}, kA2[2] = {0.875, 0}, kB1[2] = {3.125, 0};
static const double kBad[2] = {std::numeric_limits<double>::quiet_NaN(), 0};

static SignatureRule class_rule() {
  SignatureRule r;
  r.mode = 2; r.W = 2; r.thr = 0.25;
  return r;
}

static void check_class_table() {
  const SignatureRule r = class_rule();
  {   // no best class: one band per class
    PlannerMemory mem;
    ClassTable t = seed_class_table(r, 2, {}, nullptr, mem);
    CHECK(!t.has_best && mem.best_class_mode == 0);
    CHECK(t.add_if_new(kA) && !t.add_if_new(kA1) && t.add_if_new(kB) && !t.add_if_new(kBad));
    CHECK(t.classes.size() == 2);
  }
  {   // best class A, one plan in it: the seeded band is that plan
    PlannerMemory mem;
    ClassTable t = seed_class_table(r, 1, {kB, kA}, kA, mem);
    CHECK(t.has_best && mem.best_class_mode == 2 && mem.best_class == std::vector<double>(kA, kA + 2));
    CHECK(!t.add_if_new(kA1) && !t.add_if_new(kB1));
    CHECK(t.classes.size() == 2);
  }
  {   // two plans in the best class: the second member joins, the third is refused; other classes stay single
    PlannerMemory mem;
    ClassTable t = seed_class_table(r, 2, {kB, kA}, kA, mem);
    CHECK(t.add_if_new(kA1));
    CHECK(!t.add_if_new(kA2));
    CHECK(!t.add_if_new(kB1));
    CHECK(t.classes.size() == 3);
    // the remembered class outlives its band: a later table without a best band still uses it
    ClassTable later = seed_class_table(r, 2, {kA}, nullptr, mem);
    CHECK(later.has_best && later.add_if_new(kA1) && !later.add_if_new(kA2));
    // ... unless the signatures changed their kind
    SignatureRule r3 = r;
    r3.mode = 3;
    CHECK(!seed_class_table(r3, 2, {}, nullptr, mem).has_best);
  }
}

static void check_filter_class_list() {
  const SignatureRule r = class_rule();
  const std::vector<const double*> row = {kB, kA, kA1, kA2, kBad};
  const std::vector<int> order = {0, 1, 2, 3, 4};
  int kp[5], vld[5], rsn[5];
  auto is = [&](const int* v, int a, int b, int c, int d, int e) { return v[0] == a && v[1] == b && v[2] == c && v[3] == d && v[4] == e; };
  {
    PlannerMemory mem;
    filter_class_list(r, 2, order, -1, row, mem, kp, vld, rsn);
    CHECK(is(kp, 1, 1, 0, 0, 0) && is(vld, 1, 1, 1, 1, 0) && is(rsn, 1, 1, 1, 1, 1));
    CHECK(mem.best_class_mode == 0);
  }
  {   // the best band is visited first: band 2 holds class A, band 1 is the duplicate
    PlannerMemory mem;
    filter_class_list(r, 1, order, 2, row, mem, kp, vld, rsn);
    CHECK(is(kp, 1, 0, 1, 0, 0));
    CHECK(mem.best_class_mode == 2 && mem.best_class == std::vector<double>(kA1, kA1 + 2));
  }
  {   // two plans in the best class: bands 2 and 1, the third member (band 3) is refused
    PlannerMemory mem;
    filter_class_list(r, 2, order, 2, row, mem, kp, vld, rsn);
    CHECK(is(kp, 1, 1, 1, 0, 0));
  }
  {   // only the bands of `order` are written
    PlannerMemory mem;
    int k2[5] = {7, 7, 7, 7, 7};
    filter_class_list(r, 1, {1, 3}, 3, row, mem, k2, vld, rsn);
    CHECK(is(k2, 7, 0, 7, 1, 7));
  }
}

static void check_accept_in_order() {
  const SignatureRule r = class_rule();
  PlannerMemory mem;
  ClassTable t = seed_class_table(r, 1, {}, nullptr, mem);
  const double rows[10] = {1, 0, 1.125, 0, 3, 0, 5, 0, 7, 0};   // A, A1, B, and two more classes
  std::vector<int> acc;
  CHECK(accept_in_order(t, rows, 10, 5, 2, acc) == 3);   // A taken, A1 a duplicate, B fills the second slot: the rest is not examined
  CHECK((acc == std::vector<int>{10, 12}));
  CHECK(accept_in_order(t, rows, 0, 5, 0, acc) == 0 && acc.size() == 2);
}

static void check_initial_plan_and_via_points() {
  const SignatureRule r = class_rule();
  PlannerMemory mem;
  const ClassTable t = seed_class_table(r, 2, {kB, kA, kA1}, nullptr, mem);
  std::vector<int> ve;
  // without an initial plan's class
  CHECK(initial_plan_band(t, mem, 3, -1) == -1);
  CHECK(initial_plan_band(t, mem, 3, 2) == 2);
  CHECK(via_point_rule(t, mem, 3, true, false, 2, 1.0, ve) && (ve == std::vector<int>{1, 1, 1}));   // all candidates
  CHECK(!via_point_rule(t, mem, 3, false, false, 2, 1.0, ve));                                        // neither all nor an initial plan
  // with one: the stored band wins, else the first band of the class
  mem.initial_class.assign(kA, kA + 2); mem.initial_class_mode = 2;
  CHECK(initial_plan_band(t, mem, 3, -1) == 1);
  CHECK(initial_plan_band(t, mem, 3, 2) == 2);
  CHECK(initial_plan_band(t, mem, 1, -1) == -1);
  CHECK(via_point_rule(t, mem, 3, false, true, 2, 1.0, ve) && (ve == std::vector<int>{0, 1, 1}));
  CHECK(via_point_rule(t, mem, 3, true, true, 2, 1.0, ve) && (ve == std::vector<int>{1, 1, 1}));
  CHECK(!via_point_rule(t, mem, 3, true, true, 0, 1.0, ve));    // no via-points
  CHECK(!via_point_rule(t, mem, 3, true, true, 2, 0.0, ve));    // weight_viapoint <= 0
  CHECK(!via_point_rule(t, mem, 0, true, true, 2, 1.0, ve));    // no band
  // an invalid stored class is none (initial_plan_eq_class_->isValid())
  mem.initial_class.assign(kBad, kBad + 2);
  CHECK(initial_plan_band(t, mem, 3, -1) == -1);
}

struct EdgeArgs { double dnx, dny, thr, sox, soy, min_dist; int keypoint, near_u, near_v; };   // what graph_vertices fills of GraphArgs

static void check_graph_vertices() {
  teb_amd_hcp_params_t p;
  std::memset(&p, 0, sizeof p);
  p.obstacle_heading_threshold = 0.5; p.roadmap_graph_area_width = 6; p.roadmap_graph_area_length_scale = 1.0;
  const double start[3] = {0, 0, 0}, goal[3] = {8, 0, 0};
  HostObst tab;   // the vertices read the centroids only: one obstacle in front of the start, one behind it
  tab.type = {TEB_AMD_OBST_POINT, TEB_AMD_OBST_POINT};
  tab.cx = {4, -2}; tab.cy = {1, 0};
  std::vector<double> vx, vy;
  {   // lrKeyPointGraph: the obstacle in front gives centroid +- normal * dist_to_obst, the one behind nothing
    PlannerMemory mem;
    EdgeArgs g;
    p.simple_exploration = 1;
    graph_vertices(tab, start, goal, 8.0, 0.5, &p, mem.rnd, nullptr, vx, vy, g);
    CHECK((vx == std::vector<double>{0, 4, 4, 8}) && (vy == std::vector<double>{0, 1.5, 0.5, 0}));
    CHECK(g.keypoint == 1 && g.near_u == 1 && g.near_v == 2 && g.min_dist == 0.25 && g.thr == 0.5);
    CHECK(g.dnx == 1 && g.dny == 0 && g.sox == 1 && g.soy == 0);
    CHECK(mem.rnd == std::mt19937());   // no sample drawn
  }
  {   // ProbRoadmapGraph, given unit samples: area origin (0, -3), the y sample comes first
    PlannerMemory mem;
    EdgeArgs g;
    p.simple_exploration = 0; p.roadmap_graph_no_samples = 2;
    const double us[4] = {0.5, 0.25, 0.75, 0.5};
    graph_vertices(tab, start, goal, 8.0, 0.5, &p, mem.rnd, us, vx, vy, g);
    CHECK((vx == std::vector<double>{0, 2, 4, 8}) && (vy == std::vector<double>{0, 0, 1.5, 0}));
    CHECK(g.keypoint == 0 && g.near_u == -1 && g.near_v == -1 && g.min_dist == 0.5);
    CHECK(mem.rnd == std::mt19937());
  }
  {   // ... and drawn from the planner's generator: 32-bit outputs / 2^32, y before x; the generator moves on by four
    PlannerMemory mem;
    EdgeArgs g;
    graph_vertices(tab, start, goal, 8.0, 0.5, &p, mem.rnd, nullptr, vx, vy, g);
    std::mt19937 ref;
    double u[4];
    for (double& x : u) x = (double)ref() / 4294967296.0;
    CHECK(vx.size() == 4 && vx[1] == u[1] * 8 && vy[1] == -3 + u[0] * 6 && vx[2] == u[3] * 8 && vy[2] == -3 + u[2] * 6);
    CHECK(mem.rnd == ref);
  }
}

static void check_detour_rule() {
  teb_amd_hcp_params_t p;
  std::memset(&p, 0, sizeof p);
  p.detours_orientation_tolerance = 1.5; p.max_ratio_detours_duration_best_duration = 3.0;
  // found, orientation, duration, poses
  const double st[4 * 5] = {1, 0, 2, 10,   1, 0.5, 4, 10,   1, 3.0, 4, 10,   1, 0, 7, 10,   0, 0, 1, 10};
  const int opt[5] = {1, 1, 1, 1, 1};
  const std::vector<int> order = {0, 1, 2, 3, 4};
  int32_t keep[5] = {1, 1, 1, 1, 1};
  CHECK(detour_rule_runs(order, 0, keep));
  int32_t one[5] = {1, 0, 0, 0, 0}, lost[5] = {0, 1, 1, 0, 0};
  CHECK(!detour_rule_runs(order, 0, one) && !detour_rule_runs(order, 0, lost) && !detour_rule_runs(order, 9, keep));
  apply_detour_rule(order, 0, &p, st, opt, keep);   // band 2 turns away, band 3 takes 7 / 2 of the best duration, band 4 is too short
  CHECK(keep[0] == 1 && keep[1] == 1 && keep[2] == 0 && keep[3] == 0 && keep[4] == 0);
}

typedef std::vector<double> Row;
static Row row_of(const SignatureSet& s, int b) { return Row(s.row(b), s.row(b) + s.width(b)); }

static void check_signature_set() {
  {   // fixed width 2: off[b] = 2 b
    SignatureSet s;
    CHECK(s.mode == 0 && !s.fresh(2, 0, 0.0));
    CHECK((SignatureSet::fixed_width(3, 2) == std::vector<int>{0, 2, 4, 6}));
    double* v = s.reserve(SignatureSet::fixed_width(3, 2));
    CHECK(s.mode == 0 && s.values.size() == 6);   // not valid before the stamp
    for (int k = 0; k < 6; ++k) v[k] = 10 + k;
    s.stamp(2, 0.5);
    CHECK(s.mode == 2 && s.B == 3 && s.width(1) == 2 && (row_of(s, 1) == Row{12, 13}) && s.rows().size() == 3 && s.rows()[2] == s.row(2));
    // fresh: every field that can differ
    CHECK(s.fresh(2, 3, 0.5) && s.fresh(2, 3, 0.5, 6));
    CHECK(!s.fresh(3, 3, 0.5) && !s.fresh(2, 4, 0.5) && !s.fresh(2, 3, 0.25) && !s.fresh(2, 3, 0.5, 9));
    s.gather({2, 0, 1});   // a permutation
    CHECK(s.B == 3 && (s.off == std::vector<int>{0, 2, 4, 6}) && (s.values == Row{14, 15, 10, 11, 12, 13}) && s.fresh(2, 3, 0.5, 6));
    s.gather({1});         // a drop
    CHECK(s.B == 1 && (s.off == std::vector<int>{0, 2}) && (row_of(s, 0) == Row{10, 11}) && s.fresh(2, 1, 0.5, 2) && !s.fresh(2, 3, 0.5));
    s.gather({});          // an empty map
    CHECK(s.B == 0 && (s.off == std::vector<int>{0}) && s.mode == 2 && s.fresh(2, 0, 0.5, 0));
    s.clear();
    CHECK(s.mode == 0 && s.B == 0 && s.off.empty() && !s.fresh(2, 0, 0.5));
  }
  {   // ragged: bands of scenes with 3, 0 and 1 obstacles (3-D)
    SignatureSet s;
    double* v = s.reserve({0, 3, 3, 4, 7});
    for (int k = 0; k < 7; ++k) v[k] = k;
    s.stamp(3, 1.0);
    CHECK(s.B == 4 && s.width(0) == 3 && s.width(1) == 0 && s.width(2) == 1 && (row_of(s, 2) == Row{3}) && (row_of(s, 3) == Row{4, 5, 6}));
    CHECK(s.fresh(3, 4, 1.0) && s.fresh(3, 4, 1.0, 7) && !s.fresh(2, 4, 1.0));
    s.gather({3, 1, 0});   // a permutation with a drop
    CHECK(s.B == 3 && (s.off == std::vector<int>{0, 3, 3, 6}) && (s.values == Row{4, 5, 6, 0, 1, 2}));
    s.gather({1});         // only the band without values is left
    CHECK(s.B == 1 && s.width(0) == 0 && s.row(0) != nullptr);
  }
  {   // width 0: 3-D signatures without obstacles - no values, rows that are pointers all the same
    SignatureSet s;
    s.reserve(SignatureSet::fixed_width(2, 0));
    s.stamp(3, 1.0);
    CHECK(s.B == 2 && s.width(0) == 0 && s.width(1) == 0 && s.row(1) != nullptr && s.fresh(3, 2, 1.0, 0));
    s.gather({1, 0});
    CHECK(s.B == 2 && (s.off == std::vector<int>{0, 0, 0}) && s.row(0) != nullptr);
  }
  // the hsig3d launch rule: the option pins a kernel, otherwise 32768 values fill the chip
  CHECK(hsig3d_wide(TEB_AMD_HSIG3D_AUTO, 32768) && !hsig3d_wide(TEB_AMD_HSIG3D_AUTO, 32767));
  CHECK(hsig3d_wide(TEB_AMD_HSIG3D_WIDE, 1) && !hsig3d_wide(TEB_AMD_HSIG3D_SMALL, 1 << 20));
}

static void check_band_groups() {
  {   // the single scene: one group of all bands
    const BandGroups g(1, 3, nullptr);
    CHECK(g.size() == 1 && g.B == 3 && (g.of[0] == std::vector<int>{0, 1, 2}) && g.first(0) == 0);
    CHECK(g.has(0, 0) && g.has(0, 2) && !g.has(0, 3) && !g.has(0, -1));
  }
  {   // three interleaved scenes, scene 1 without bands
    const int scene_of[5] = {2, 0, 2, 0, 2};
    const BandGroups g(3, 5, scene_of);
    CHECK(g.size() == 3 && (g.of[0] == std::vector<int>{1, 3}) && g.of[1].empty() && (g.of[2] == std::vector<int>{0, 2, 4}));
    CHECK(g.first(0) == 1 && g.first(1) == -1 && g.first(2) == 0);
    CHECK(g.has(0, 3) && !g.has(0, 2) && !g.has(1, 0) && !g.has(1, -1) && g.has(2, 4) && !g.has(2, 5));
  }
  CHECK(BandGroups(1, 0, nullptr).first(0) == -1);
}

static void check_filter_class_lists() {   // two planners over one ragged set: each sees its own bands, rows and memory
  SignatureSet s;
  const double v[8] = {1, 0, 3, 0, 1.125, 0, 3.125, 0};   // A, B, A1, B1
  std::copy(v, v + 8, s.reserve(SignatureSet::fixed_width(4, 2)));
  s.stamp(2, 1.0);
  const int scene_of[4] = {0, 1, 0, 1};
  const BandGroups g(2, 4, scene_of);
  PlannerMemory mem[2];
  int32_t kp[4], vld[4], rsn[4];
  const int32_t best[2] = {2, -1};
  filter_class_lists(s, g, 0.25, 1, best, mem, kp, vld, rsn);   // scene 0: band 2 first, band 0 its duplicate; scene 1: band 1, then its duplicate
  CHECK(kp[0] == 0 && kp[1] == 1 && kp[2] == 1 && kp[3] == 0 && vld[0] && vld[3] && rsn[1]);
  CHECK(mem[0].best_class_mode == 2 && (mem[0].best_class == Row{1.125, 0}) && mem[1].best_class_mode == 0);
  filter_class_lists(s, BandGroups(1, 4, nullptr), 0.25, 1, nullptr, mem, kp, vld, rsn);   // one planner: A, B kept; mem[0] still holds class A
  CHECK(kp[0] == 1 && kp[1] == 1 && kp[2] == 0 && kp[3] == 0);
}

// teb_amd_compact_bands as it stood before compaction_map, the single scene's loop
static void old_single_compaction(int B, const int32_t* keep, int best, std::vector<int>& map, int& new_best) {
  std::vector<int> order(B);
  for (int b = 0; b < B; ++b) order[b] = b;
  const bool has_best = best >= 0 && best < B;
  if (has_best) std::swap(order[0], order[best]);
  map.clear();
  for (int k = 0; k < B; ++k) if (keep[order[k]]) map.push_back(order[k]);
  new_best = has_best && keep[best] ? 0 : -1;
}

static void check_compaction_map() {
  typedef std::vector<int> V;
  V map;
  int32_t nb[3];
  {   // one group of four bands
    const BandGroups g(1, 4, nullptr);
    const int32_t all[4] = {1, 1, 1, 1}, some[4] = {1, 0, 1, 1}, none[4] = {0, 0, 0, 0};
    int32_t best = 0;
    compaction_map(g, all, &best, map, nb);
    CHECK((map == V{0, 1, 2, 3}) && nb[0] == 0);              // best = 0: nothing moves
    best = 3;
    compaction_map(g, all, &best, map, nb);
    CHECK((map == V{3, 1, 2, 0}) && nb[0] == 0);              // best = the last band: swapped with the first
    compaction_map(g, some, &best, map, nb);
    CHECK((map == V{3, 2, 0}) && nb[0] == 0);                 // ... kept
    best = 1;
    compaction_map(g, some, &best, map, nb);
    CHECK((map == V{0, 2, 3}) && nb[0] == -1);                // best not kept: the swap still happened (1 <-> 0), no new best
    best = 4;
    compaction_map(g, some, &best, map, nb);
    CHECK((map == V{0, 2, 3}) && nb[0] == -1);                // out of range: none
    best = -1;
    compaction_map(g, all, &best, map, nullptr);
    CHECK((map == V{0, 1, 2, 3}));
    compaction_map(g, all, nullptr, map, nb);
    CHECK((map == V{0, 1, 2, 3}) && nb[0] == -1);             // all kept, no best
    best = 2;
    compaction_map(g, none, &best, map, nb);
    CHECK(map.empty() && nb[0] == -1);                        // none kept
  }
  {   // three interleaved groups: scene 0 = {1, 3}, scene 1 empty, scene 2 = {0, 2, 4, 5}; best bands 3 and 4, band 4 dropped
    const int scene_of[6] = {2, 0, 2, 0, 2, 2};
    const BandGroups g(3, 6, scene_of);
    const int32_t keep[6] = {1, 1, 0, 1, 0, 1}, best[3] = {3, -1, 4};
    compaction_map(g, keep, best, map, nb);   // order after the swaps 1 <-> 3 and 0 <-> 4: 4 3 2 1 0 5
    CHECK((map == V{3, 1, 0, 5}) && nb[0] == 0 && nb[1] == -1 && nb[2] == -1);
    const int32_t all[6] = {1, 1, 1, 1, 1, 1}, none[6] = {0, 0, 0, 0, 0, 0};
    compaction_map(g, all, best, map, nb);
    CHECK((map == V{4, 3, 2, 1, 0, 5}) && nb[0] == 1 && nb[1] == -1 && nb[2] == 0);
    const int32_t foreign[3] = {0, 1, 3};     // bands of other groups: none
    compaction_map(g, all, foreign, map, nb);
    CHECK((map == V{0, 1, 2, 3, 4, 5}) && nb[0] == -1 && nb[1] == -1 && nb[2] == -1);
    compaction_map(g, none, best, map, nb);
    CHECK(map.empty() && nb[0] == -1 && nb[2] == -1);
  }
  {   // one group against the single scene's former loop, 200 seeded keep / best draws
    std::mt19937 rnd(7);
    for (int draw = 0; draw < 200; ++draw) {
      const int B = 1 + (int)(rnd() % 8);
      int32_t keep[8];
      for (int b = 0; b < B; ++b) keep[b] = rnd() % 3 != 0;
      const int32_t best = (int)(rnd() % (B + 4)) - 2;   // -2 .. B + 1: out of range on both sides too
      V old_map;
      int old_best;
      old_single_compaction(B, keep, best, old_map, old_best);
      compaction_map(BandGroups(1, B, nullptr), keep, &best, map, nb);
      CHECK(map == old_map && nb[0] == old_best);
    }
  }
}

int main() {
  check_signature_set();
  check_band_groups();
  check_filter_class_lists();
  check_compaction_map();
  check_path_enumerator();
  check_take_paths();
  check_predicates();
  check_class_table();
  check_filter_class_list();
  check_accept_in_order();
  check_initial_plan_and_via_points();
  check_graph_vertices();
  check_detour_rule();
  if (g_failures == 0) std::printf("hcp host check ok\n");
  return g_failures;
}
