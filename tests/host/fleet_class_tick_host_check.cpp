// fleet_class_tick_host_check.cpp — the rules csrc/teb_fleet_host.hpp adds for the _per_class calls (no HIP): which configuration field
// feeds which argument of a tick (scene_tick_params) and the feasibility specs of a fleet (check_feasibility_specs,
// feasibility_spec_of), against answers written out by hand. Stand-alone: tests/test_fleet_class_tick_host.py compiles it with the
// address and undefined-behaviour sanitizers and runs it; it prints what failed and returns the number of failures.
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

// class k: every field a tick reads has its own value, 100 k + a field number, so that a swapped field cannot hide
static teb_amd_config_t cls(int k) {
  teb_amd_config_t c;
  std::memset(&c, 0, sizeof c);
  const double o = 100.0 * k;
  c.min_obstacle_dist = o + 1; c.max_vel_x = o + 2; c.max_vel_theta = o + 3; c.acc_lim_x = o + 4; c.min_samples = 100 * k + 5;
  c.weight_viapoint = o + 6; c.selection_obst_cost_scale = o + 7; c.selection_viapoint_cost_scale = o + 8;
  c.selection_alternative_time_cost = k % 2;
  // neighbours that must NOT be read in their place
  c.inflation_dist = o + 11; c.max_vel_x_backwards = o + 12; c.max_vel_y = o + 13; c.acc_lim_theta = o + 14; c.max_samples = 100 * k + 15;
  c.weight_obstacle = o + 16; c.selection_cost_hysteresis = o + 17; c.selection_prefer_initial_plan = o + 18;
  return c;
}

static void check_tick_params() {
  const std::vector<teb_amd_config_t> c = {cls(0), cls(1), cls(2)};
  const int of[] = {2, 0, 1, 1, 2};
  for (int s = 0; s < 5; ++s) {
    const SceneTickParams p = scene_tick_params(c.data(), 3, of, s);
    const double o = 100.0 * of[s];
    CHECK(p.dist_to_obst == o + 1);       // min_obstacle_dist, not inflation_dist
    CHECK(p.max_vel_x == o + 2);          // not max_vel_x_backwards / max_vel_y
    CHECK(p.max_vel_theta == o + 3);
    CHECK(p.acc_lim_x == o + 4);          // not acc_lim_theta
    CHECK(p.min_samples == 100 * of[s] + 5);   // not max_samples
    CHECK(p.weight_viapoint == o + 6);
    CHECK(p.obst_cost_scale == o + 7);    // the selection_ scales, not the hysteresis / the preference
    CHECK(p.viapoint_cost_scale == o + 8);
    CHECK(p.alternative_time_cost == of[s] % 2);
  }
  // without a map: the table of one class, whatever the scene
  for (int s = 0; s < 5; ++s) {
    const SceneTickParams p = scene_tick_params(c.data() + 1, 1, nullptr, s);
    CHECK(p.dist_to_obst == 101 && p.min_samples == 105 && p.alternative_time_cost == 1 && p.viapoint_cost_scale == 108);
  }
}

static teb_amd_feasibility_spec_t spec(int nf, const double* x, const double* y, double radius = 0.2, double angle = 0.5, int idx = -1, double dist = -1) {
  teb_amd_feasibility_spec_t q;
  q.n_footprint = nf; q.footprint_x = x; q.footprint_y = y; q.inscribed_radius = radius; q.min_resolution_collision_check_angular = angle;
  q.look_ahead_idx = idx; q.feasibility_check_lookahead_distance = dist;
  return q;
}
static bool refused(const FeasibilitySpecs& r, int k, int s, const char* word) {
  return !r.refusal.ok() && r.refusal.spec == k && r.refusal.scene == s && std::strstr(r.refusal.why, word) && r.offset.empty();
}

static void check_specs() {
  std::vector<double> x(64, 0.0), y(64, 0.0);
  const int kMax = 64;
  // a rectangle, a triangle, a single vertex: offsets 0, 4, 7, 8
  std::vector<teb_amd_feasibility_spec_t> q = {spec(4, x.data(), y.data()), spec(3, x.data(), y.data()), spec(1, x.data(), y.data())};
  const int of[] = {0, 1, 2, 2, 1, 0};
  FeasibilitySpecs r = check_feasibility_specs(q.data(), 3, of, 6, 1, kMax);
  CHECK(r.refusal.ok() && r.refusal.spec == -1 && r.refusal.scene == -1);
  CHECK(r.offset == (std::vector<int>{0, 4, 7, 8}));
  // the limits of a footprint: 1 and 64 pass, 0 and 65 are refused with the spec named
  q[1].n_footprint = 64;
  r = check_feasibility_specs(q.data(), 3, of, 6, 1, kMax);
  CHECK(r.refusal.ok() && r.offset == (std::vector<int>{0, 4, 68, 69}));
  q[1].n_footprint = 65;
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 1, -1, "n_footprint"));
  q[1].n_footprint = 0;
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 1, -1, "n_footprint"));
  q[1].n_footprint = 3;
  // null arrays, the radius, the angle - the FIRST offending spec
  q[2].footprint_y = nullptr;
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 2, -1, "null footprint"));
  q[0].footprint_x = nullptr;
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 0, -1, "null footprint"));
  q[0].footprint_x = x.data(); q[2].footprint_y = y.data();
  q[1].inscribed_radius = 0;
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 1, -1, "must be > 0"));
  q[1].inscribed_radius = 0.0 / 1.0 - 1;   // negative
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 1, -1, "must be > 0"));
  q[1].inscribed_radius = 0.2; q[2].min_resolution_collision_check_angular = 0;
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 2, -1, "must be > 0"));
  const double nan = std::strtod("nan", nullptr);
  q[2].min_resolution_collision_check_angular = nan;   // !(x > 0)
  CHECK(refused(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax), 2, -1, "must be > 0"));
  q[2].min_resolution_collision_check_angular = 0.5;
  CHECK(check_feasibility_specs(q.data(), 3, of, 6, 1, kMax).refusal.ok());
  // no spec at all
  CHECK(refused(check_feasibility_specs(q.data(), 0, of, 6, 1, kMax), -1, -1, "at least one"));
  CHECK(refused(check_feasibility_specs(nullptr, 3, of, 6, 1, kMax), -1, -1, "at least one"));
  // the range of spec_of_scene: the first offending scene
  const int high[] = {0, 1, 3, 5, 0, 0}, neg[] = {0, 1, 2, 2, -1, 0};
  CHECK(refused(check_feasibility_specs(q.data(), 3, high, 6, 1, kMax), -1, 2, "not one of the specs"));
  CHECK(refused(check_feasibility_specs(q.data(), 3, neg, 6, 1, kMax), -1, 4, "not one of the specs"));
  CHECK(check_feasibility_specs(q.data(), 3, neg, 4, 1, kMax).refusal.ok());   // (the offending entry is not part of the set)
  // a bad spec comes before a bad map
  q[0].n_footprint = 0;
  CHECK(refused(check_feasibility_specs(q.data(), 3, high, 6, 1, kMax), 0, -1, "n_footprint"));
  q[0].n_footprint = 4;
  // the NULL map: one spec per class of the map, one without a map; with a map given the class count does not matter
  CHECK(check_feasibility_specs(q.data(), 3, nullptr, 6, 3, kMax).refusal.ok());
  CHECK(check_feasibility_specs(q.data(), 3, nullptr, 6, 3, kMax).offset == (std::vector<int>{0, 4, 7, 8}));
  CHECK(refused(check_feasibility_specs(q.data(), 3, nullptr, 6, 2, kMax), -1, -1, "one spec per class"));
  CHECK(refused(check_feasibility_specs(q.data(), 3, nullptr, 6, 1, kMax), -1, -1, "one spec per class"));
  CHECK(refused(check_feasibility_specs(q.data(), 2, nullptr, 6, 3, kMax), -1, -1, "one spec per class"));
  CHECK(check_feasibility_specs(q.data(), 1, nullptr, 6, 1, kMax).refusal.ok());
  CHECK(check_feasibility_specs(q.data(), 3, of, 6, 7, kMax).refusal.ok());
  // which spec a scene takes
  const int cls_of[] = {2, 2, 0, 1, 1, 0};
  for (int s = 0; s < 6; ++s) {
    CHECK(feasibility_spec_of(of, cls_of, s) == of[s]);          // the call's map wins
    CHECK(feasibility_spec_of(nullptr, cls_of, s) == cls_of[s]);  // else the class
    CHECK(feasibility_spec_of(nullptr, nullptr, s) == 0);         // else the one spec
    CHECK(feasibility_spec_of(of, nullptr, s) == of[s]);
  }
}

int main() {
  check_tick_params();
  check_specs();
  if (g_failures == 0) std::printf("fleet class tick host check ok\n");
  return g_failures;
}
