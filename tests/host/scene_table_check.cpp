// scene_table_check.cpp — the host part of csrc/teb_scene_store.hpp on its own (no HIP): HostObst::append against the parse of the
// hand-concatenated input, the segments of a scene set against the running sums written out as numbers, derive_scene_lists on a table
// with dynamic and circular rows. Stand-alone: tests/test_scene_table_host.py compiles it with the address and undefined-behaviour
// sanitizers and runs it; it prints what failed and returns the number of failures.
#define TEB_SCENE_STORE_HOST_ONLY
#include "../../teb_local_planner_amd/csrc/teb_scene_store.hpp"

#include <cstdio>
#include <cstring>
#include <string>

using namespace tebamd;

static int g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

// the caller's side of an obstacle table
struct Input {
  std::vector<int32_t> type, dynamic, vert_offset;
  std::vector<double> ax, ay, bx, by, radius, vx, vy, vert_x, vert_y;
  teb_amd_obstacles_t c() const {
    teb_amd_obstacles_t o{};
    o.count = (int32_t)type.size();
    o.type = type.data(); o.ax = ax.data(); o.ay = ay.data(); o.bx = bx.data(); o.by = by.data(); o.radius = radius.data();
    o.vx = vx.data(); o.vy = vy.data(); o.dynamic = dynamic.data();
    o.vert_offset = vert_offset.data(); o.vert_x = vert_x.data(); o.vert_y = vert_y.data();
    return o;
  }
};

static HostObst parsed(const Input& in) {
  HostObst t;
  const teb_amd_obstacles_t o = in.c();
  if (const char* bad = parse_obstacle_table(&o, t)) { std::printf("FAILED parse: %s\n", bad); ++g_failures; }
  return t;
}

static bool same_table(const HostObst& a, const HostObst& b) {
  bool same = true;
  for_each_column(a, b, [&](const auto& x, const auto& y, ColumnExtent) {
    same = same && x.size() == y.size() && (x.empty() || std::memcmp(x.data(), y.data(), x.size() * sizeof(x[0])) == 0);
  });
  return same;
}

// three points / circles, one of them dynamic
static Input points() {
  Input p;
  p.type = {TEB_AMD_OBST_POINT, TEB_AMD_OBST_CIRCULAR, TEB_AMD_OBST_POINT};
  p.ax = {1.0, 3.0, 5.0}; p.ay = {2.0, 4.0, 6.0}; p.bx = {0, 0, 0}; p.by = {0, 0, 0}; p.radius = {0.0, 0.5, 0.0};
  p.vx = {0.0, 0.1, 0.0}; p.vy = {0.0, -0.2, 0.0}; p.dynamic = {0, 1, 0};
  p.vert_offset = {0, 0, 0, 0};
  return p;
}
// triangle, line, quadrilateral, pill: 7 vertices
static Input polygons() {
  Input p;
  p.type = {TEB_AMD_OBST_POLYGON, TEB_AMD_OBST_LINE, TEB_AMD_OBST_POLYGON, TEB_AMD_OBST_PILL};
  p.ax = {0.0, -1.0, 0.0, 2.0}; p.ay = {0.0, -1.0, 0.0, 2.5}; p.bx = {0.0, -2.0, 0.0, 3.0}; p.by = {0.0, -1.5, 0.0, 2.5};
  p.radius = {0.0, 0.0, 0.0, 0.2}; p.vx = {0.0, 0.0, 0.3, 0.0}; p.vy = {0.0, 0.0, 0.1, 0.0}; p.dynamic = {0, 0, 1, 0};
  p.vert_offset = {0, 3, 3, 7, 7};
  p.vert_x = {0.0, 1.0, 0.0, 4.0, 5.0, 5.0, 4.0}; p.vert_y = {0.0, 0.0, 1.0, 4.0, 4.0, 5.5, 5.0};
  return p;
}

static void check_append() {
  const HostObst P = parsed(points()), G = parsed(polygons()), E = parsed(Input{});
  CHECK(P.rows() == 3 && P.verts() == 0 && P.voff.size() == 4);
  CHECK(G.rows() == 4 && G.verts() == 7 && G.voff == (std::vector<int>{0, 3, 3, 7, 7}));
  CHECK(E.rows() == 0 && E.voff == std::vector<int>{0});

  // points ++ polygons ++ empty, the input concatenated by hand
  Input in;
  in.type = {TEB_AMD_OBST_POINT, TEB_AMD_OBST_CIRCULAR, TEB_AMD_OBST_POINT, TEB_AMD_OBST_POLYGON, TEB_AMD_OBST_LINE, TEB_AMD_OBST_POLYGON, TEB_AMD_OBST_PILL};
  in.ax = {1.0, 3.0, 5.0, 0.0, -1.0, 0.0, 2.0}; in.ay = {2.0, 4.0, 6.0, 0.0, -1.0, 0.0, 2.5};
  in.bx = {0, 0, 0, 0.0, -2.0, 0.0, 3.0}; in.by = {0, 0, 0, 0.0, -1.5, 0.0, 2.5};
  in.radius = {0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.2}; in.vx = {0.0, 0.1, 0.0, 0.0, 0.0, 0.3, 0.0}; in.vy = {0.0, -0.2, 0.0, 0.0, 0.0, 0.1, 0.0};
  in.dynamic = {0, 1, 0, 0, 0, 1, 0};
  in.vert_offset = {0, 0, 0, 0, 3, 3, 7, 7};
  in.vert_x = {0.0, 1.0, 0.0, 4.0, 5.0, 5.0, 4.0}; in.vert_y = {0.0, 0.0, 1.0, 4.0, 4.0, 5.5, 5.0};
  HostObst t = P;
  t.append(G);
  t.append(E);
  CHECK(same_table(t, parsed(in)));
  CHECK(t.voff == (std::vector<int>{0, 0, 0, 0, 3, 3, 7, 7}));

  // polygons ++ empty ++ points ++ polygons: the offsets of what follows move by the 7 vertices already held
  Input in2 = polygons();
  const Input p = points(), g = polygons();
  for (const Input* q : {&p, &g}) {
    in2.type.insert(in2.type.end(), q->type.begin(), q->type.end()); in2.dynamic.insert(in2.dynamic.end(), q->dynamic.begin(), q->dynamic.end());
    in2.ax.insert(in2.ax.end(), q->ax.begin(), q->ax.end()); in2.ay.insert(in2.ay.end(), q->ay.begin(), q->ay.end());
    in2.bx.insert(in2.bx.end(), q->bx.begin(), q->bx.end()); in2.by.insert(in2.by.end(), q->by.begin(), q->by.end());
    in2.radius.insert(in2.radius.end(), q->radius.begin(), q->radius.end());
    in2.vx.insert(in2.vx.end(), q->vx.begin(), q->vx.end()); in2.vy.insert(in2.vy.end(), q->vy.begin(), q->vy.end());
    in2.vert_x.insert(in2.vert_x.end(), q->vert_x.begin(), q->vert_x.end()); in2.vert_y.insert(in2.vert_y.end(), q->vert_y.begin(), q->vert_y.end());
  }
  in2.vert_offset = {0, 3, 3, 7, 7, 7, 7, 7, 10, 10, 14, 14};
  HostObst u = G;
  u.append(E);
  u.append(P);
  u.append(G);
  CHECK(same_table(u, parsed(in2)));
  CHECK(u.voff == (std::vector<int>{0, 3, 3, 7, 7, 7, 7, 7, 10, 10, 14, 14}));
}

static bool segment_is(const SceneSegment& g, size_t row, size_t voff, size_t vert, size_t via, size_t list) {
  return g.row == row && g.voff == voff && g.vert == vert && g.via == via && g.list == list;
}

// 4 scenes: E (no rows), P (3 rows), G (4 rows, 7 vertices), Q (2 rows) with the empty scene first, in the middle and last. Row offset
// ro = rows before the scene, offsets ro + s, vertices vo, via-points wo, cache list 5 ro.
static void check_segments() {
  const HostObst P = parsed(points()), G = parsed(polygons()), E = parsed(Input{});
  Input two = points();
  for (auto* v : {&two.type, &two.dynamic}) v->pop_back();
  for (auto* v : {&two.ax, &two.ay, &two.bx, &two.by, &two.radius, &two.vx, &two.vy}) v->pop_back();
  two.vert_offset.pop_back();
  const HostObst Q = parsed(two);
  CHECK(Q.rows() == 2);
  {
    const HostObst tabs[] = {E, P, G, Q};
    const int via[] = {0, 2, 1, 0};
    const std::vector<SceneSegment> s = scene_segments(tabs, via, 4);
    CHECK(segment_is(s[0], 0, 0, 0, 0, 0)); CHECK(segment_is(s[1], 0, 1, 0, 0, 0));
    CHECK(segment_is(s[2], 3, 5, 0, 2, 15)); CHECK(segment_is(s[3], 7, 10, 7, 3, 35));
  }
  {
    const HostObst tabs[] = {P, G, E, Q};
    const int via[] = {2, 1, 0, 0};
    const std::vector<SceneSegment> s = scene_segments(tabs, via, 4);
    CHECK(segment_is(s[0], 0, 0, 0, 0, 0)); CHECK(segment_is(s[1], 3, 4, 0, 2, 15));
    CHECK(segment_is(s[2], 7, 9, 7, 3, 35)); CHECK(segment_is(s[3], 7, 10, 7, 3, 35));
  }
  {
    const HostObst tabs[] = {P, G, Q, E};
    const int via[] = {2, 1, 0, 4};
    const std::vector<SceneSegment> s = scene_segments(tabs, via, 4);
    CHECK(segment_is(s[0], 0, 0, 0, 0, 0)); CHECK(segment_is(s[1], 3, 4, 0, 2, 15));
    CHECK(segment_is(s[2], 7, 9, 7, 3, 35)); CHECK(segment_is(s[3], 9, 12, 7, 3, 45));
    // the columns one after the other: every scene finds its own rows, offsets (still local) and vertices at its segment
    HostObst all;
    for (const HostObst& t : tabs) all.append_segment(t);
    CHECK(all.rows() == 9 && all.voff.size() == 9 + 4 && all.verts() == 7);
    for (int k = 0; k < 4; ++k) {
      const HostObst& t = tabs[k];
      CHECK(std::equal(t.voff.begin(), t.voff.end(), all.voff.begin() + s[k].voff));
      CHECK(std::equal(t.ax.begin(), t.ax.end(), all.ax.begin() + s[k].row));
      CHECK(std::equal(t.brad.begin(), t.brad.end(), all.brad.begin() + s[k].row));
      CHECK(std::equal(t.pvx.begin(), t.pvx.end(), all.pvx.begin() + s[k].vert));
    }
  }
}

// rows: 0 point, 1 circle r 0.5 (dynamic), 2 point (dynamic), 3 circle r `r3`, 4 point whose radius entry (0.7) must not reach the cache
static Input five(double r3) {
  Input p;
  p.type = {TEB_AMD_OBST_POINT, TEB_AMD_OBST_CIRCULAR, TEB_AMD_OBST_POINT, TEB_AMD_OBST_CIRCULAR, TEB_AMD_OBST_POINT};
  p.ax = {1, 3, 5, 7, 9}; p.ay = {2, 4, 6, 8, 10}; p.bx = {0, 0, 0, 0, 0}; p.by = {0, 0, 0, 0, 0}; p.radius = {0.0, 0.5, 0.0, r3, 0.7};
  p.vx = {0.0, 0.1, 0.3, 0.0, 0.0}; p.vy = {0.0, -0.2, 0.4, 0.0, 0.0}; p.dynamic = {0, 1, 1, 0, 0};
  p.vert_offset = {0, 0, 0, 0, 0, 0};
  return p;
}

static void check_lists() {
  teb_amd_config_t cfg;
  std::memset(&cfg, 0, sizeof cfg);
  SceneLists d;
  using VI = std::vector<int>;
  using VD = std::vector<double>;
  const HostObst t = parsed(five(0.25));

  cfg.include_dynamic_obstacles = 1;
  derive_scene_lists(cfg, t, d);
  CHECK(d.st == (VI{0, 3, 4}) && d.dy == (VI{1, 2}));
  CHECK(d.static_radius_zero == 0 && d.pointlike_rows);
  CHECK(d.lo == (VD{1, 7, 9, 3, 5, /* y */ 2, 8, 10, 4, 6, /* radius */ 0, 0.25, 0, 0.5, 0, /* vx */ 0, 0, 0, 0.1, 0.3, /* vy */ 0, 0, 0, -0.2, 0.4}));

  cfg.include_dynamic_obstacles = 0;
  derive_scene_lists(cfg, t, d);
  CHECK(d.st == (VI{0, 1, 2, 3, 4}) && d.dy.empty());
  CHECK(d.static_radius_zero == 0 && d.pointlike_rows);
  CHECK(d.lo == (VD{1, 3, 5, 7, 9, 2, 4, 6, 8, 10, 0, 0.5, 0, 0.25, 0, 0, 0.1, 0.3, 0, 0, 0, -0.2, 0.4, 0, 0}));

  // the only circle with a radius is dynamic: the static list has none exactly when the dynamic obstacles have a list of their own
  const HostObst z = parsed(five(0.0));
  cfg.include_dynamic_obstacles = 1;
  derive_scene_lists(cfg, z, d);
  CHECK(d.static_radius_zero == 1 && d.st == (VI{0, 3, 4}));
  cfg.include_dynamic_obstacles = 0;
  derive_scene_lists(cfg, z, d);
  CHECK(d.static_radius_zero == 0);

  // a row that is neither a point nor a circle; no rows at all
  derive_scene_lists(cfg, parsed(polygons()), d);
  CHECK(!d.pointlike_rows && d.lo.size() == 20);
  derive_scene_lists(cfg, parsed(Input{}), d);
  CHECK(d.pointlike_rows && d.static_radius_zero == 1 && d.st.empty() && d.dy.empty() && d.lo.empty());
}

static void check_parse_errors() {
  Input p = polygons();
  p.vert_offset = {0, 0, 0, 4, 4};   // the triangle has no vertices
  HostObst t;
  teb_amd_obstacles_t o = p.c();
  const char* bad = parse_obstacle_table(&o, t);
  CHECK(bad && std::string(bad) == "polygon obstacle without vertices");
  p = points();
  p.type[1] = 17;
  o = p.c();
  bad = parse_obstacle_table(&o, t);
  CHECK(bad && std::string(bad) == "unknown obstacle type");
}

int main() {
  check_append();
  check_segments();
  check_lists();
  check_parse_errors();
  if (g_failures == 0) std::printf("scene table check ok\n");
  return g_failures;
}
