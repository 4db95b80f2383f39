// fleet_config_host_check.cpp — csrc/teb_fleet_host.hpp on its own (no HIP): the host rules of a fleet with robot classes against
// answers written out by hand. Stand-alone: tests/test_fleet_config_host.py compiles it with the address and undefined-behaviour
// sanitizers and runs it; it prints what failed and returns the number of failures.
//
// The LDS plan is the synthetic one of launch_host_check.cpp, so that every threshold can be worked out in a comment:
//   bytes(S, layout, cache) = per_pose[layout] * S + 8 * cache, per_pose = 100 (blocks), 50 (LDS band), 10 (band in HBM)
// against a limit of 20000 B.
#include "../../teb_local_planner_amd/csrc/teb_fleet_host.hpp"

#include <cstdio>
#include <cstring>
#include <vector>

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

// a class: analytic Jacobians, dynamic obstacles on, autoResize on, the given footprint
static teb_amd_config_t cls(int footprint, int dynamic = 1, int jacobian = TEB_AMD_JACOBIAN_ANALYTIC, int autosize = 1) {
  teb_amd_config_t c;
  std::memset(&c, 0, sizeof c);
  c.footprint_type = footprint; c.include_dynamic_obstacles = dynamic; c.jacobian_mode = jacobian; c.teb_autosize = autosize;
  return c;
}
static bool refused(const ClassRefusal& r, int k, const char* field) { return r.cls == k && r.field && std::strcmp(r.field, field) == 0 && r.why; }

static void check_agreement() {
  std::vector<teb_amd_config_t> c = {cls(TEB_AMD_FOOTPRINT_POINT), cls(TEB_AMD_FOOTPRINT_POLYGON), cls(TEB_AMD_FOOTPRINT_LINE)};
  CHECK(fleet_classes_agree(c.data(), 3).ok());
  CHECK(fleet_classes_agree(c.data(), 1).ok());
  // footprints, limits and weights may differ; jacobian_mode and include_dynamic_obstacles may not
  c[2].include_dynamic_obstacles = 0;
  CHECK(refused(fleet_classes_agree(c.data(), 3), 2, "include_dynamic_obstacles"));
  CHECK(fleet_classes_agree(c.data(), 2).ok());   // (the offending class is not part of the list)
  c[2].include_dynamic_obstacles = 7;             // a truth value: 7 agrees with 1
  CHECK(fleet_classes_agree(c.data(), 3).ok());
  c[0].include_dynamic_obstacles = 0; c[1].include_dynamic_obstacles = 0;
  CHECK(refused(fleet_classes_agree(c.data(), 3), 2, "include_dynamic_obstacles"));   // all off but the last: it is the one that differs from class 0
  c[2].include_dynamic_obstacles = 0;
  CHECK(fleet_classes_agree(c.data(), 3).ok());   // all off agrees as well
  // a numeric-Jacobian class is refused wherever it stands - also alone, also when every class is numeric
  c[1].jacobian_mode = TEB_AMD_JACOBIAN_G2O_NUMERIC;
  CHECK(refused(fleet_classes_agree(c.data(), 3), 1, "jacobian_mode"));
  c[0].jacobian_mode = TEB_AMD_JACOBIAN_G2O_NUMERIC;
  CHECK(refused(fleet_classes_agree(c.data(), 3), 0, "jacobian_mode"));
  CHECK(refused(fleet_classes_agree(c.data(), 1), 0, "jacobian_mode"));
  // the first offending class is named, and of its fields the Jacobian mode first
  std::vector<teb_amd_config_t> d = {cls(0), cls(0, 0, TEB_AMD_JACOBIAN_G2O_NUMERIC), cls(0, 0)};
  CHECK(refused(fleet_classes_agree(d.data(), 3), 1, "jacobian_mode"));
  d[1].jacobian_mode = TEB_AMD_JACOBIAN_ANALYTIC;
  CHECK(refused(fleet_classes_agree(d.data(), 3), 1, "include_dynamic_obstacles"));
  // the class of every scene
  const int of[] = {0, 2, 1, 2};
  CHECK(first_scene_without_class(of, 4, 3) == -1);
  CHECK(first_scene_without_class(of, 4, 2) == 1);
  CHECK(first_scene_without_class(of, 1, 1) == -1);
  const int neg[] = {0, 1, -1};
  CHECK(first_scene_without_class(neg, 3, 2) == 2);
  CHECK(first_scene_without_class(neg, 2, 2) == -1);
  CHECK(first_scene_without_class(neg, 0, 2) == -1);
}

static TableLayout table(bool rows, const std::vector<teb_amd_config_t>& c, int M, int stride = 150, int created = LAYOUT_BLOCKS, bool generic = false,
                         int pin = TEB_AMD_LAYOUT_AUTO) {
  return fleet_layout_per_table(rows, c.data(), (int)c.size(), generic, created, pin, M, stride, kLimit, plan_bytes);
}

static void check_distance_path() {
  const std::vector<teb_amd_config_t> pts = {cls(TEB_AMD_FOOTPRINT_POINT), cls(TEB_AMD_FOOTPRINT_CIRCULAR), cls(TEB_AMD_FOOTPRINT_POINT)};
  CHECK(fleet_footprints_pointlike(pts.data(), 3));
  // classes x tables: point-like iff the rows of every table AND the footprint of every class are
  TableLayout t = table(true, pts, 100);
  CHECK(t.fast_points == 1 && t.cache_entries == 100 && t.layout == LAYOUT_BLOCKS && !t.hbm_band);
  t = table(false, pts, 100);   // one table holds a line or a polygon
  CHECK(t.fast_points == 0 && t.cache_entries == 0);
  for (int shape : {TEB_AMD_FOOTPRINT_TWO_CIRCLES, TEB_AMD_FOOTPRINT_LINE, TEB_AMD_FOOTPRINT_POLYGON})
    for (int where = 0; where < 3; ++where) {   // ONE class with a shape, wherever it stands in the list
      std::vector<teb_amd_config_t> c = pts;
      c[where].footprint_type = shape;
      CHECK(!fleet_footprints_pointlike(c.data(), 3));
      t = table(true, c, 100);
      CHECK(t.fast_points == 0 && t.cache_entries == 0 && t.layout == LAYOUT_BLOCKS);
      CHECK(fleet_footprints_pointlike(c.data(), where) == true);   // (the classes in front of it are point-like)
    }
  // one class is the single scene of a handle: the rule of layout_per_table itself
  for (int shape = TEB_AMD_FOOTPRINT_POINT; shape <= TEB_AMD_FOOTPRINT_POLYGON; ++shape) {
    const std::vector<teb_amd_config_t> one = {cls(shape)};
    const TableLayout a = table(true, one, 100), b = layout_per_table(true, shape, false, LAYOUT_BLOCKS, TEB_AMD_LAYOUT_AUTO, 100, 150, kLimit, plan_bytes);
    CHECK(a.fast_points == b.fast_points && a.cache_entries == b.cache_entries && a.layout == b.layout && a.hbm_band == b.hbm_band);
    CHECK(a.fast_points == (shape == TEB_AMD_FOOTPRINT_POINT || shape == TEB_AMD_FOOTPRINT_CIRCULAR));
  }
  // the cache of the widest table: blocks, 150 poses: 15000 + 8 M <= 20000 up to M = 625
  CHECK(table(true, pts, 625).fast_points == 1);
  CHECK(table(true, pts, 626).fast_points == 0);
  CHECK(table(true, pts, 0).fast_points == 0);   // no rows anywhere: nothing to cache
  // an LDS band of 390 poses (19500 B) holds a cache of 62 entries; a wider one moves the band to HBM (3900 + 8 M) and keeps the cache
  t = table(true, pts, 62, 390, LAYOUT_BAND);
  CHECK(t.fast_points == 1 && t.layout == LAYOUT_BAND && !t.hbm_band);
  t = table(true, pts, 63, 390, LAYOUT_BAND);
  CHECK(t.fast_points == 1 && t.layout == LAYOUT_BAND_HBM && t.hbm_band && t.cache_entries == 63);
  std::vector<teb_amd_config_t> poly = pts;
  poly[1].footprint_type = TEB_AMD_FOOTPRINT_POLYGON;
  t = table(true, poly, 63, 390, LAYOUT_BAND);   // a generic fleet has no cache to make room for: the band stays in LDS
  CHECK(t.fast_points == 0 && t.layout == LAYOUT_BAND && !t.hbm_band);
  // teb_amd_options_t::generic_distance_path: the generic path whatever the classes and tables are
  t = table(true, pts, 100, 150, LAYOUT_BLOCKS, true);
  CHECK(t.fast_points == 0 && t.cache_entries == 0);
}

static void check_autosize() {
  std::vector<teb_amd_config_t> c = {cls(0, 1, 0, 0), cls(0, 1, 0, 0), cls(0, 1, 0, 0)};
  CHECK(!fleet_any_autosize(c.data(), 3));
  c[2].teb_autosize = 1;
  CHECK(fleet_any_autosize(c.data(), 3));
  CHECK(!fleet_any_autosize(c.data(), 2));
  c[2].teb_autosize = 0; c[0].teb_autosize = 1;
  CHECK(fleet_any_autosize(c.data(), 1));
}

int main() {
  check_agreement();
  check_distance_path();
  check_autosize();
  if (g_failures == 0) std::printf("fleet config host check ok\n");
  return g_failures;
}
