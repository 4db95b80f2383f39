// teb_hcp_host.hpp — the host rules of ONE HomotopyClassPlanner (src/homotopy_class_planner.cpp, src/graph_search.cpp, h_signature.h),
// free of HIP: what its planner remembers between ticks, the class list, the depth-first path order, the vertices of its graph, the
// steps of an exploration tick that are decisions rather than arithmetic on bands, and the detour rule. teb_amd.hip calls them for the
// single scene (one planner) and for a scene set (one planner per scene); the device steps between them are the routes of teb_amd.hip.
// Compiles with a plain host compiler when teb_scene_store.hpp comes in TEB_SCENE_STORE_HOST_ONLY mode: tests/host/hcp_host_check.cpp.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <random>
#include <utility>
#include <vector>

#include "teb_scene_store.hpp"

namespace tebamd {

// isValid / isEqual of HSignature and HSignature3d (h_signature.h:190-226, 349-409) and the "reasonable" test of renewAndAnalyzeOldTebs
// on rows of W doubles: mode 2 = HSignature (W = 2), mode 3 = HSignature3d (W = obstacles of the planner)
struct SignatureRule {
  int mode = 2, W = 2;
  double thr = 0.1;   // h_signature_threshold
  static int sign_of(double z) { return z == 0 ? 0 : (z < 0 ? -1 : 1); }
  bool valid(const double* v) const { for (int k = 0; k < W; ++k) if (!std::isfinite(v[k])) return false; return true; }
  bool reasonable(const double* v) const { if (mode == 2) return true; for (int k = 0; k < W; ++k) if (v[k] > 1.0) return false; return true; }
  bool equal(const double* a, const double* b) const {   // a.isEqual(b)
    if (mode == 2) return std::fabs(b[0] - a[0]) <= thr && std::fabs(b[1] - a[1]) <= thr;   // h_signature.h:196-204
    for (int i = 0; i < W; ++i) {                                                             // h_signature.h:360-377
      if (std::fabs(b[i]) < thr || std::fabs(a[i]) < thr) continue;   // far-away obstacle: ignored
      if (sign_of(b[i]) != sign_of(a[i])) return false;
    }
    return true;
  }
};

// What a planner - the single scene's, or a robot of a fleet - remembers between ticks
struct PlannerMemory {
  std::vector<double> best_class;      // best_teb_eq_class_: signature of the last best band; outlives the band
  int best_class_mode = 0;             // 0 = none yet, 2 / 3 = HSignature / HSignature3d
  std::vector<double> initial_class;   // initial_plan_eq_class_: signature of the band made from the last initial plan
  int initial_class_mode = 0;
  std::mt19937 rnd;                    // ProbRoadmapGraph::rnd_generator_ (graph_search.h:211): default-seeded 32-bit Mersenne twister
  std::vector<double> g_vx, g_vy;      // the graph of the last exploration (empty: it returned before its graph)
  std::vector<unsigned char> g_adj;
  bool has_best(const SignatureRule& r) const { return best_class_mode == r.mode && (int)best_class.size() == r.W; }
  bool has_initial(const SignatureRule& r) const { return initial_class_mode == r.mode && (int)initial_class.size() == r.W && r.valid(initial_class.data()); }
  void forget_graph() { g_vx.clear(); g_vy.clear(); g_adj.clear(); }
};

// equivalence_classes_ of one planner with addEquivalenceClassIfNew
struct ClassTable {
  SignatureRule sig;
  int max_in_best = 1;                        // max_number_plans_in_current_class
  std::vector<std::vector<double>> classes;   // equivalence_classes_
  bool has_best = false;
  std::vector<double> best;                   // best_teb_eq_class_
  bool add_if_new(const double* v) {   // addEquivalenceClassIfNew, src/homotopy_class_planner.cpp:189-212
    if (!sig.valid(v)) return false;   // "Ignoring invalid H-signature"
    bool has = false;
    for (const auto& c : classes) if (sig.equal(v, c.data())) { has = true; break; }
    if (has) {   // isInBestTebClass / numTebsInBestTebClass use best_teb_eq_class_, which outlives the band it was computed from (:385-410)
      const bool in_best = has_best && sig.equal(best.data(), v);
      int count = 0;
      if (has_best) for (const auto& c : classes) if (sig.equal(best.data(), c.data())) ++count;
      if (!in_best || count >= max_in_best) return false;
    }
    classes.emplace_back(v, v + sig.W);
    return true;
  }
};

// The class table at the start of a tick: a class per row (the signatures of the planner's bands, in band order); best_row, if any,
// becomes the remembered best class (best_teb_eq_class_ = calculateEquivalenceClass(best_teb_), :224-227), which the table then uses
inline ClassTable seed_class_table(const SignatureRule& r, int max_in_best, const std::vector<const double*>& rows, const double* best_row,
                                   PlannerMemory& mem) {
  ClassTable t;
  t.sig = r; t.max_in_best = max_in_best;
  for (const double* v : rows) t.classes.emplace_back(v, v + r.W);
  if (best_row) { mem.best_class.assign(best_row, best_row + r.W); mem.best_class_mode = r.mode; }
  if (mem.has_best(r)) { t.has_best = true; t.best = mem.best_class; }
  return t;
}

// The class list of renewAndAnalyzeOldTebs over the bands `order` (band indices, in band order) of ONE planner: the single scene's
// bands, or the bands of one scene of a set. row[b]: the W values of band b. best: a band of `order` that is visited first
// (std::iter_swap with the first band) and whose class becomes the remembered best class, or anything else for none.
// kp / vld / rsn [band index], each or NULL, are written for the bands of `order` only.
inline void filter_class_list(const SignatureRule& r, int max_number_plans_in_current_class, std::vector<int> order, int best,
                              const std::vector<const double*>& row, PlannerMemory& mem, int32_t* kp, int32_t* vld, int32_t* rsn) {
  for (int b : order) { if (vld) vld[b] = r.valid(row[b]); if (rsn) rsn[b] = r.reasonable(row[b]); }
  const auto at = std::find(order.begin(), order.end(), best);
  if (at != order.end()) std::iter_swap(order.begin(), at);
  ClassTable t = seed_class_table(r, max_number_plans_in_current_class, {}, at != order.end() ? row[best] : nullptr, mem);
  for (int b : order) { const bool keep = t.add_if_new(row[b]); if (kp) kp[b] = keep; }
}

// GraphSearchInterface::DepthFirst (src/graph_search.cpp:45-91) as a resumable generator of start-goal paths in the reference's order
struct PathEnumerator {
  std::vector<std::vector<int>> adj;
  int goal = 0;
  struct Frame { int v; int phase; size_t k; };
  std::vector<Frame> stack;
  std::vector<int> visited;
  std::vector<char> on_path;
  int64_t expansions = 0, max_expansions = 0;   // > 0: give up after that many vertex expansions (dead-end subtrees can be exponential)
  PathEnumerator() = default;
  PathEnumerator(std::vector<std::vector<int>> a, int start, int goal_) : adj(std::move(a)), goal(goal_), on_path(adj.size(), 0) {
    stack.push_back({start, 0, 0}); visited.push_back(start); on_path[start] = 1;
  }
  bool next(std::vector<int>& path) {
    while (!stack.empty()) {
      if (max_expansions > 0 && ++expansions > max_expansions) return false;
      Frame& f = stack.back();
      const std::vector<int>& out = adj[f.v];
      if (f.phase == 0) {       // first loop: the goal, if adjacent, closes one path
        f.phase = 1; f.k = 0;
        if (std::find(out.begin(), out.end(), goal) != out.end()) { path = visited; path.push_back(goal); return true; }
      }
      bool descended = false;
      while (f.k < out.size()) {   // second loop: recursion into every adjacent vertex not yet on the path
        const int w = out[f.k++];
        if (on_path[w] || w == goal) continue;
        visited.push_back(w); on_path[w] = 1;
        stack.push_back({w, 0, 0});
        descended = true;
        break;
      }
      if (descended) continue;
      on_path[f.v] = 0; visited.pop_back(); stack.pop_back();
    }
    return false;
  }
};

// the out-edges of every vertex from the adjacency byte matrix [N * N], in the add_edge order of the double loop
inline std::vector<std::vector<int>> adjacency_lists(const unsigned char* m, int N) {
  std::vector<std::vector<int>> adj(N);
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) if (m[(size_t)i * N + j]) adj[i].push_back(j);
  return adj;
}

// The paths of one planner's graph over the rounds of a tick: candidates examined so far, and whether more may come
struct PathSource {
  PathEnumerator en;
  int64_t examined = 0;
  bool more = false;
  PathSource() = default;
  PathSource(std::vector<std::vector<int>> adj, int64_t max_paths) : en(std::move(adj), 0, 0), more(true) {
    en.goal = (int)en.adj.size() - 1;
    if (max_paths > 0) en.max_expansions = max_paths * 10000;
  }
};
// Up to `limit` further paths in depth-first order, not beyond the budget of max_paths (> 0) examined paths: their vertices appended to
// px / py, their ends to off. Returns how many, or -1 at a path of more than max_vertices vertices (it fits no band).
inline int take_paths(PathSource& ps, int limit, int64_t max_paths, int max_vertices, const std::vector<double>& vx, const std::vector<double>& vy,
                      std::vector<double>& px, std::vector<double>& py, std::vector<int>& off) {
  std::vector<int> path;
  int count = 0;
  while (count < limit && (max_paths <= 0 || ps.examined + count < max_paths)) {
    if (!ps.en.next(path)) { ps.more = false; break; }
    if ((int)path.size() > max_vertices) return -1;
    for (int v : path) { px.push_back(vx[v]); py.push_back(vy[v]); }
    off.push_back((int)px.size());
    ++count;
  }
  if (max_paths > 0 && ps.examined + count >= max_paths) ps.more = false;
  return count;
}

// First come first served: the classified candidates first .. first + count - 1 of one planner (signature rows of W values from
// rows on, in path order) against its `room` free slots; the accepted ones are appended to acc. Returns how many were examined.
inline int accept_in_order(ClassTable& t, const double* rows, int first, int count, int room, std::vector<int>& acc) {
  int examined = 0, taken = 0;
  for (int k = 0; k < count && taken < room; ++k) {
    ++examined;
    if (t.add_if_new(rows + (size_t)k * t.sig.W)) { acc.push_back(first + k); ++taken; }
  }
  return examined;
}

// getInitialPlanTEB (:495-536) over the n_bands bands of the planner (classes of t, in band order): the band created from the initial
// plan in this tick (created >= 0), else the first band of the remembered initial plan's class, else -1
inline int initial_plan_band(const ClassTable& t, const PlannerMemory& mem, int n_bands, int created) {
  if (created >= 0 || !mem.has_initial(t.sig)) return created;
  for (int b = 0; b < n_bands && b < (int)t.classes.size(); ++b)
    if (t.sig.equal(t.classes[b].data(), mem.initial_class.data())) return b;
  return -1;
}

// updateReferenceTrajectoryViaPoints (:286-315): false when the rule leaves the bands as they are - no band, no via-points, no weight,
// or neither viapoints_all_candidates nor an initial plan; else ve[b] of the planner's n_bands bands: all of them, or exactly those
// of the initial plan's class
inline bool via_point_rule(const ClassTable& t, const PlannerMemory& mem, int n_bands, bool all_candidates, bool has_plan, int n_via,
                           double weight_viapoint, std::vector<int>& ve) {
  if (n_bands <= 0 || (!all_candidates && !has_plan) || n_via <= 0 || weight_viapoint <= 0) return false;
  ve.assign(n_bands, 1);
  if (all_candidates) return true;
  const bool have_initial_class = mem.has_initial(t.sig);
  for (int b = 0; b < n_bands; ++b)
    ve[b] = have_initial_class && b < (int)t.classes.size() && t.sig.equal(mem.initial_class.data(), t.classes[b].data());
  return true;
}

// The vertices of createGraph for ONE planner, on the host (O(M) on the centroids of its obstacle table): lrKeyPointGraph
// (src/graph_search.cpp:115-153) or ProbRoadmapGraph (:247-290, samples from unit_samples or drawn from the planner's generator).
// vx / vy: start, key points or samples, goal. ga (GraphArgs of teb_graph.hpp, or any struct with these members): what the edge test
// needs beside them - dnx, dny, thr, keypoint, near_u, near_v (key points of the obstacle nearest to the start, or -1), sox, soy, min_dist.
template <class EdgeArgs>
void graph_vertices(const HostObst& hob, const double* start, const double* goal, double start_goal_dist, double dist_to_obst,
                    const teb_amd_hcp_params_t* p, std::mt19937& generator, const double* unit_samples, std::vector<double>& vx,
                    std::vector<double>& vy, EdgeArgs& ga) {
  const int M = (int)hob.rows();
  const double sx = start[0], sy = start[1], gx = goal[0], gy = goal[1];
  double dfx = gx - sx, dfy = gy - sy;
  auto normalize = [](double& x, double& y) { const double z = x * x + y * y; if (z > 0) { const double n = std::sqrt(z); x = x / n; y = y / n; } };
  vx.assign(1, sx); vy.assign(1, sy);
  ga.keypoint = p->simple_exploration ? 1 : 0; ga.near_u = ga.near_v = -1; ga.thr = p->obstacle_heading_threshold;
  ga.sox = std::cos(start[2]); ga.soy = std::sin(start[2]);
  if (p->simple_exploration) {                                              // lrKeyPointGraph::createGraph, :115-153
    double nx = -dfy, ny = dfx;
    normalize(nx, ny);
    nx = nx * dist_to_obst; ny = ny * dist_to_obst;
    normalize(dfx, dfy);
    double min_dist = std::numeric_limits<double>::max();
    for (int o = 0; o < M; ++o) {
      const double ox = hob.cx[o] - sx, oy = hob.cy[o] - sy;
      const double dist = std::sqrt(ox * ox + oy * oy);
      if ((ox * dfx + oy * dfy) / dist < 0.1) continue;                     // obstacle not in front of the start
      vx.push_back(hob.cx[o] + nx); vy.push_back(hob.cy[o] + ny);
      vx.push_back(hob.cx[o] - nx); vy.push_back(hob.cy[o] - ny);
      if (p->obstacle_heading_threshold && dist < min_dist) { min_dist = dist; ga.near_u = (int)vx.size() - 2; ga.near_v = (int)vx.size() - 1; }
    }
    ga.min_dist = 0.5 * dist_to_obst;
  } else {                                                                  // ProbRoadmapGraph::createGraph, :247-290
    double nx = -dfy, ny = dfx;
    normalize(nx, ny);
    const double area_width = p->roadmap_graph_area_width;
    const double len = start_goal_dist * p->roadmap_graph_area_length_scale;
    const double phi = std::atan2(dfy, dfx);
    double ox, oy;
    if (p->roadmap_graph_area_length_scale != 1.0) {
      double ux = dfx, uy = dfy;
      normalize(ux, uy);
      const double f = 0.5 * (1.0 - p->roadmap_graph_area_length_scale) * start_goal_dist, w2 = 0.5 * area_width;
      ox = (sx + f * ux) - w2 * nx; oy = (sy + f * uy) - w2 * ny;
    } else {
      const double w2 = 0.5 * area_width;
      ox = sx - w2 * nx; oy = sy - w2 * ny;
    }
    normalize(dfx, dfy);
    int drawn = 0;
    auto draw = [&](double a, double b) {    // boost::random::uniform_real_distribution<double>(a, b) on the 32-bit engine
      if (unit_samples) return unit_samples[drawn++] * (b - a) + a;
      for (;;) {
        const double numerator = (double)(generator() - std::mt19937::min());
        const double divisor = (double)(std::mt19937::max() - std::mt19937::min()) + 1;
        const double result = numerator / divisor * (b - a) + a;
        if (result < b) return result;
      }
    };
    const double cphi = std::cos(phi), sphi = std::sin(phi);
    for (int i = 0; i < p->roadmap_graph_no_samples; ++i) {
      const double uy = draw(0, area_width);   // GCC evaluates Eigen::Vector2d(distribution_x(g), distribution_y(g)) right to left
      const double ux = draw(0, len);
      vx.push_back(ox + (cphi * ux - sphi * uy)); vy.push_back(oy + (sphi * ux + cphi * uy));
    }
    ga.min_dist = dist_to_obst;
  }
  vx.push_back(gx); vy.push_back(gy);
  ga.dnx = dfx; ga.dny = dfy;
}

// deletePlansDetouringBackwards over the bands `order` of ONE planner (src/homotopy_class_planner.cpp:760-820), in two halves: whether
// the rule runs at all - it needs two kept bands and a kept best one - and the rule over the statistics of detour_stats_kernel
// (st [4 * band]) and the optimized flags (opt [band]).
inline bool detour_rule_runs(const std::vector<int>& order, int best, const int32_t* keep) {
  int kept = 0;
  for (int b : order) kept += keep[b] != 0;
  return kept >= 2 && std::find(order.begin(), order.end(), best) != order.end() && keep[best];   // "a moving direction wasn't chosen yet", :769-773
}
inline void apply_detour_rule(const std::vector<int>& order, int best, const teb_amd_hcp_params_t* p, const double* st, const int* opt, int32_t* keep) {
  auto found = [&](int b) { return st[4 * b] != 0; };
  auto orient = [&](int b) { return st[4 * b + 1]; };
  auto duration = [&](int b) { return st[4 * b + 2]; };
  auto poses = [&](int b) { return (int)st[4 * b + 3]; };
  if (poses(best) < 2) return;
  const double best_plan_duration = std::max(duration(best), 1.0);
  if (!found(best)) return;   // the plan is shorter than len_orientation_vector
  auto normalize_theta = [](double theta) {   // g2o::normalize_theta (misc.h)
    if (theta >= -M_PI && theta < M_PI) return theta;
    const double multiplier = std::floor(theta / (2 * M_PI));
    theta = theta - multiplier * 2 * M_PI;
    if (theta >= M_PI) theta -= 2 * M_PI;
    if (theta < -M_PI) theta += 2 * M_PI;
    return theta;
  };
  for (int b : order) {
    if (!keep[b] || b == best) continue;
    if (poses(b) < 2 || !found(b)) { keep[b] = 0; continue; }
    if (std::fabs(normalize_theta(orient(b) - orient(best))) > p->detours_orientation_tolerance) { keep[b] = 0; continue; }
    if (!opt[b]) { keep[b] = 0; continue; }
    if (duration(b) / best_plan_duration > p->max_ratio_detours_duration_best_duration) { keep[b] = 0; continue; }
  }
}

// The signatures of the B bands of a handle as the compute calls leave them: band b holds values [off[b], off[b + 1]). A table of
// fixed width W (the single scene) is the offset form with off[b] = b * W; the bands of a scene set have the widths of their scenes.
struct SignatureSet {
  int mode = 0, B = 0;   // mode 0 = no valid signatures, 2 / 3 = HSignature / HSignature3d
  double prescaler = 0;  // h_signature_prescaler of those signatures
  std::vector<int> off;  // [B + 1]
  std::vector<double> values;
  static std::vector<int> fixed_width(int B, int W) { std::vector<int> o(B + 1); for (int b = 0; b <= B; ++b) o[b] = b * W; return o; }
  const double* row(int b) const { return values.data() + off[b]; }
  int width(int b) const { return off[b + 1] - off[b]; }
  std::vector<const double*> rows() const { std::vector<const double*> r(B); for (int b = 0; b < B; ++b) r[b] = row(b); return r; }
  void clear() { mode = 0; B = 0; off.clear(); values.clear(); }
  // The two halves of a compute call: room for the values at the given offsets (never empty, so that row() of a set without values
  // is a pointer), not valid before stamp() says of what the downloaded values are
  double* reserve(std::vector<int> offsets) { clear(); off = std::move(offsets); values.assign(std::max(off.back(), 1), 0.0); return values.data(); }
  void stamp(int mode_, double prescaler_) { mode = mode_; B = (int)off.size() - 1; prescaler = prescaler_; }
  // Are these the signatures of B_ bands in mode mode_ at that prescaler? n_values >= 0: and that many values in all (the single scene:
  // B * W, which in mode 3 is the row count of the table they were computed against)
  bool fresh(int mode_, int B_, double prescaler_, long long n_values = -1) const {
    return mode != 0 && mode == mode_ && B == B_ && prescaler == prescaler_ && (n_values < 0 || off.back() == n_values);
  }
  void gather(const std::vector<int>& map) {   // band k becomes the former band map[k]
    std::vector<int> o(1, 0);
    std::vector<double> v;
    for (int b : map) { v.insert(v.end(), row(b), row(b) + width(b)); o.push_back((int)v.size()); }
    if (v.empty()) v.assign(1, 0.0);
    off.swap(o); values.swap(v); B = (int)map.size();
  }
};

// The hsig3d launch rule: one lane per (band, obstacle) when the values fill the chip, otherwise lanes over (obstacle, segment) - same
// bits, lower latency. option: teb_amd_options_t::hsig3d_kernel, which pins one of the two kernels (tests, tools/hsig_bench.py).
inline bool hsig3d_wide(int option, long long n_values) {
  return option == TEB_AMD_HSIG3D_WIDE || (option != TEB_AMD_HSIG3D_SMALL && n_values >= 32768);
}

// The planners of a handle and their bands: the bands 0 .. B - 1 in groups, one per planner. group_of NULL: one group of all bands (the
// single scene); else band b belongs to group group_of[b] < n_groups (a scene set: band -> scene).
struct BandGroups {
  int B = 0;
  std::vector<std::vector<int>> of;   // the bands of every group, in band order
  BandGroups() = default;
  BandGroups(int n_groups, int B_, const int* group_of) : B(B_), of(n_groups) {
    for (int b = 0; b < B; ++b) of[group_of ? group_of[b] : 0].push_back(b);
  }
  int size() const { return (int)of.size(); }
  int first(int g) const { return of[g].empty() ? -1 : of[g].front(); }
  bool has(int g, int b) const { return std::binary_search(of[g].begin(), of[g].end(), b); }
};

// The class list of renewAndAnalyzeOldTebs for every planner (filter_class_list): memory [groups], best [groups] or NULL for none
inline void filter_class_lists(const SignatureSet& S, const BandGroups& G, double threshold, int max_number_plans_in_current_class, const int32_t* best,
                               PlannerMemory* memory, int32_t* kp, int32_t* vld, int32_t* rsn) {
  const std::vector<const double*> row = S.rows();
  for (int g = 0; g < G.size(); ++g)   // (a planner without bands: its width is not looked at)
    filter_class_list(SignatureRule{S.mode, G.of[g].empty() ? 0 : S.width(G.first(g)), threshold}, max_number_plans_in_current_class, G.of[g],
                      best ? best[g] : -1, row, memory[g], kp, vld, rsn);
}

// The erase of the dropped bands with the order renewAndAnalyzeOldTebs leaves: std::iter_swap(tebs_.begin(), it_best_teb) inside every
// planner's bands (best [groups] or NULL; a best[g] that is no band of group g is none), then the kept bands in the resulting order.
// map: the former index of every new band. new_best [groups] or NULL: the new index of every kept best band, else -1.
inline void compaction_map(const BandGroups& G, const int32_t* keep, const int32_t* best, std::vector<int>& map, int32_t* new_best) {
  std::vector<int> order(G.B), group(G.B, 0);
  for (int g = 0; g < G.size(); ++g) for (int b : G.of[g]) group[b] = g;
  for (int b = 0; b < G.B; ++b) order[b] = b;
  auto is_best = [&](int b) { return best && best[group[b]] == b; };
  for (int g = 0; g < G.size(); ++g) {
    if (new_best) new_best[g] = -1;
    if (best && G.has(g, best[g])) std::swap(order[G.first(g)], order[best[g]]);
  }
  map.clear();
  for (int b : order) {
    if (!keep[b]) continue;
    if (new_best && is_best(b)) new_best[group[b]] = (int)map.size();
    map.push_back(b);
  }
}

}  // namespace tebamd
