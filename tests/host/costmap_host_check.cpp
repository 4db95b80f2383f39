// costmap_host_check.cpp — csrc/teb_costmap_host.hpp on its own (no HIP): the host rules of the costmap-to-obstacles conversion against
// answers worked out by hand. Stand-alone: tests/test_costmap_host.py compiles it with the address and undefined-behaviour sanitizers
// and runs it; it prints what failed and returns the number of failures. Coordinates are small integers or binary fractions, so every
// expected value is exact.
#define TEB_SCENE_STORE_HOST_ONLY
#include "../../teb_local_planner_amd/csrc/teb_costmap_host.hpp"

#include <cstdio>
#include <string>

using namespace tebamd;

static int g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

typedef std::vector<int> Ints;
typedef std::vector<double> Reals;

static GridDev grid(int sx, int sy) { return GridDev{nullptr, sx, sy, 0.5, 0.0, 0.0}; }
static bool refused(const Refusal& r, int code, const char* text) { return r.code == code && r.text && std::string(r.text) == text; }

static void check_lane_rule() {
  CHECK(point_lanes(1, 37).lanes() == 0 && point_lanes(1, 37).ncols == 0 && point_lanes(1, 37).nrows == 0);
  CHECK(point_lanes(41, 1).lanes() == 0);
  CmoLanes l = point_lanes(2, 2);
  CHECK(l.ncols == 1 && l.nrows == 1 && l.chunk == 4 && l.nchunks == 1 && l.lanes() == 1);
  l = point_lanes(120, 120);
  CHECK(l.ncols == 119 && l.nrows == 119 && l.chunk == 4 && l.nchunks == 30 && l.lanes() == 3570);
  l = point_lanes(257, 1025);   // 256 columns x 256 chunks: exactly 64 K lanes stay at 4 rows per lane
  CHECK(l.chunk == 4 && l.lanes() == 65536);
  l = point_lanes(257, 1026);
  CHECK(l.chunk == 8 && l.nchunks == 129);
  l = point_lanes(1000, 1000);
  CHECK(l.chunk == 16 && l.nchunks == 63 && l.lanes() == 62937);
  l = point_lanes(4097, 4097);   // the chunk stops at 64: the lanes grow
  CHECK(l.chunk == 64 && l.nchunks == 64 && l.lanes() == 262144);
}

static void check_block_geometry() {
  CmpGeom q;
  CHECK(polygon_blocks(120, 120, 1, q) == 119 && q.k == 4096 && q.ncols == 119 && q.nrows == 119 && q.T == 1 && q.nty == 119 && q.nby == 1);
  CHECK(polygon_blocks(120, 120, 3, q) == 40 && q.k == 455 && q.nty == 40 && q.nby == 1);
  CHECK(polygon_blocks(120, 120, 8, q) == 15 && q.k == 64 && q.nty == 15 && q.nby == 1);
  CHECK(polygon_blocks(120, 120, 64, q) == 4 && q.k == 1 && q.nty == 2 && q.nby == 2);
  CHECK(polygon_blocks(1, 37, 8, q) == 0 && q.nty == 0 && q.nby == 0);
  CHECK(polygon_blocks(41, 1, 8, q) == 0);
  // 2^20 columns x (4096 * 1024) rows of single cells: 2^20 x 1024 = 2^30 blocks is the most; one more column is too many
  CHECK(polygon_blocks((1 << 20) + 1, 4096 * 1024 + 1, 1, q) == (1LL << 30) && q.nby == 1024);
  CHECK(polygon_blocks((1 << 20) + 2, 4096 * 1024 + 1, 1, q) == -1);
}

static void check_filter() {
  const double at0[3] = {1.5, -2.0, 0.0}, at[3] = {0.25, 4.0, 0.3};
  CmoFilter f = costmap_filter(at0, 1.25);
  CHECK(f.rx == 1.5 && f.ry == -2.0 && f.c == 1.0 && f.s == 0.0 && f.dist == 1.25);
  f = costmap_filter(at, 0.0);
  CHECK(f.c == std::cos(0.3) && f.s == std::sin(0.3));
}

// the kernels' search for the scene of a flat block (cmp_scene_of_block, teb_costmap_polygons.hpp): the last s with blk0[s] <= b
static int scene_of_block(const Ints& blk0, int b) {
  int lo = 0, hi = (int)blk0.size() - 1;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk0[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

static void check_set_layout() {
  const double poses[9] = {0, 0, 0, 1, 1, 0, 2, 2, 0};
  const SceneInputs none;
  {   // points: lanes + 1 counters per scene, a grid without lanes in the middle keeps its one counter
    const GridDev g[3] = {grid(120, 120), grid(1, 37), grid(2, 2)};
    PointRows K;
    CHECK(!K.layout(g, 3, poses, 0.5, nullptr));
    CHECK(K.counters == 3574 && K.max_lanes == 3570 && K.rec.size() == 3 && (K.tot == Ints{0, 0, 0}));
    CHECK(K.rec[0].cnt_off == 0 && K.rec[1].cnt_off == 3571 && K.rec[2].cnt_off == 3572);
    CHECK(K.rec[1].ncols == 0 && K.rec[1].nrows == 0 && K.rec[1].nchunks == 0 && K.rec[1].chunk == 4);
    CHECK(K.rec[2].ncols == 1 && K.rec[2].nchunks == 1 && K.rec[2].g.sx == 2 && K.rec[2].f.rx == 2.0 && K.rec[2].f.dist == 0.5 && K.rec[2].out_off == 0);
    K.tot = {7, 0, 1};
    int32_t n[3] = {-1, -1, -1};
    CHECK(!K.place(none, SceneCaps{8, 0, 0}, PointRows::Out{n, nullptr, nullptr, 0}));
    CHECK(K.rows == 8 && K.rec[0].out_off == 0 && K.rec[1].out_off == 7 && K.rec[2].out_off == 7 && n[0] == 7 && n[1] == 0 && n[2] == 1 && K.px.size() == 8);
    // one row too many: the counts are reported, the call is refused
    n[0] = n[1] = n[2] = -1;
    CHECK(refused(K.place(none, SceneCaps{7, 0, 0}, PointRows::Out{n, nullptr, nullptr, 0}), TEB_AMD_ERR_CAPACITY,
                  "costmap cells + custom obstacles exceed max_obstacles") && n[0] == 7 && n[2] == 1);
    K.tot = {INT_MAX, INT_MAX, 5};   // the prefixes saturate, the sum does not: refused before any launch reads them
    CHECK(refused(K.place(none, SceneCaps{(size_t)INT_MAX, 0, 0}, PointRows::Out{nullptr, nullptr, nullptr, 0}), TEB_AMD_ERR_CAPACITY,
                  "costmap cells + custom obstacles exceed max_obstacles"));
    CHECK(K.rows == 2 * (size_t)INT_MAX + 5 && K.rec[1].out_off == INT_MAX && K.rec[2].out_off == INT_MAX);
    // 2^15 columns x 2^15 chunks of 64 rows: 2^30 lanes. One such grid fits the int counters, two do not
    const GridDev big[2] = {grid((1 << 15) + 1, (1 << 21) + 1), grid((1 << 15) + 1, (1 << 21) + 1)};
    PointRows one, two;
    CHECK(!one.layout(big, 1, poses, 0.5, nullptr) && one.counters == (1u << 30) + 1);
    CHECK(refused(two.layout(big, 2, poses, 0.5, nullptr), TEB_AMD_ERR_CAPACITY, "the grids of the set are too large for one call"));
  }
  {   // polygons: the blocks of the scenes in one flat list; the search skips the scene without blocks
    const GridDev g[3] = {grid(120, 120), grid(1, 37), grid(9, 12)};
    const int32_t tiles[3] = {8, 1, 8};
    PolygonRows K;
    CHECK(!K.layout(g, 3, poses, 0.5, tiles));
    CHECK((K.blk0 == Ints{0, 15, 15, 16}) && K.blocks == 16 && K.ncnt == 19 && K.tot.size() == 9);
    CHECK(K.rec[0].blk0 == 0 && K.rec[0].nblk == 15 && K.rec[0].cnt0 == 0 && K.rec[0].q.k == 64);
    CHECK(K.rec[1].blk0 == 15 && K.rec[1].nblk == 0 && K.rec[1].cnt0 == 16 && K.rec[1].q.k == 4096);
    CHECK(K.rec[2].blk0 == 15 && K.rec[2].nblk == 1 && K.rec[2].cnt0 == 17 && K.rec[2].q.ncols == 8 && K.rec[2].q.nrows == 11 && K.rec[2].f.ry == 2.0);
    CHECK(scene_of_block(K.blk0, 0) == 0 && scene_of_block(K.blk0, 14) == 0 && scene_of_block(K.blk0, 15) == 2);
    K.tot = {4, 0, 2, /* vertices */ 9, 0, 5, /* polygon vertices */ 6, 0, 4};
    int32_t no[3] = {-1, -1, -1}, np[3] = {-1, -1, -1};
    const PolygonRows::Out out{no, np, nullptr, nullptr, nullptr, 0, 0};
    CHECK(!K.place(none, SceneCaps{6, 10, 0}, out));
    CHECK(K.rows == 6 && K.verts == 14 && K.pverts == 10 && K.off.size() == 7 && K.px.size() == 14 && K.py.size() == 14);
    CHECK(no[0] == 4 && no[1] == 0 && no[2] == 2 && np[0] == 9 && np[1] == 0 && np[2] == 5);
    CHECK(K.rec[0].row0 == 0 && K.rec[1].row0 == 4 && K.rec[2].row0 == 4 && K.rec[0].vtx0 == 0 && K.rec[1].vtx0 == 9 && K.rec[2].vtx0 == 9);
    // rows are refused before polygon vertices; both after the counts are out
    no[0] = np[0] = -1;
    CHECK(refused(K.place(none, SceneCaps{5, 9, 0}, out), TEB_AMD_ERR_CAPACITY, "converted costmap rows + custom obstacles exceed max_obstacles") && no[0] == 4);
    CHECK(refused(K.place(none, SceneCaps{6, 9, 0}, out), TEB_AMD_ERR_CAPACITY, "more polygon vertices than max_obstacle_vertices") && np[0] == 9);
    K.tot = {INT_MAX, 1, 1, INT_MAX, INT_MAX, 1, 0, 0, 0};   // saturating prefixes, refused
    CHECK(refused(K.place(none, SceneCaps{(size_t)INT_MAX, 0, 0}, out), TEB_AMD_ERR_CAPACITY, "converted costmap rows + custom obstacles exceed max_obstacles"));
    CHECK(K.rows == (long long)INT_MAX + 2 && K.verts == 2LL * INT_MAX + 1);
    CHECK(K.rec[1].row0 == INT_MAX && K.rec[2].row0 == INT_MAX && K.rec[1].vtx0 == INT_MAX && K.rec[2].vtx0 == INT_MAX);
    // a grid of more than 2^30 blocks is refused as such; two grids of 2^29 blocks need 3 (2^30 + 2) counters: too many for one call
    const GridDev big[2] = {grid((1 << 19) + 1, (1 << 22) + 1), grid((1 << 19) + 1, (1 << 22) + 1)};
    const GridDev wide[1] = {grid((1 << 20) + 2, (1 << 22) + 1)};
    const int32_t ones[2] = {1, 1};
    PolygonRows one, two, three;
    CHECK(!one.layout(big, 1, poses, 0.5, ones) && one.blocks == (1 << 29) && one.ncnt == (1 << 29) + 1);
    CHECK(refused(two.layout(big, 2, poses, 0.5, ones), TEB_AMD_ERR_CAPACITY, "the grids of the set are too large for one call"));
    CHECK(refused(three.layout(wide, 1, poses, 0.5, ones), TEB_AMD_ERR_CAPACITY, "grid too large"));
  }
}

// a table over arrays that live as long as the check that uses it
struct Table {
  Ints type, voff;
  Reals ax, ay, rad, vx, vy;
  teb_amd_obstacles_t view() {
    teb_amd_obstacles_t o{};
    o.count = (int)type.size(); o.type = type.data(); o.ax = ax.data(); o.ay = ay.data(); o.radius = rad.empty() ? nullptr : rad.data();
    o.vert_offset = voff.empty() ? nullptr : voff.data(); o.vert_x = vx.empty() ? nullptr : vx.data(); o.vert_y = vy.empty() ? nullptr : vy.data();
    return o;
  }
};

static void check_input_parse() {
  Table two{{TEB_AMD_OBST_POINT, TEB_AMD_OBST_CIRCULAR}, {}, {1, 2}, {3, 4}, {0, 0.5}, {}, {}};
  Table tri{{TEB_AMD_OBST_POLYGON}, {0, 3}, {0}, {0}, {}, {0, 4, 0}, {0, 0, 4}};
  Table bare{{TEB_AMD_OBST_POLYGON}, {}, {0}, {0}, {}, {}, {}};   // a polygon without vertex arrays
  const SceneCaps roomy{100, 100, 100};
  const double vx[5] = {1, 2, 3, 4, 5}, vy[5] = {5, 4, 3, 2, 1};
  SceneInputs in;
  {   // a zeroed table among real ones, via totals
    const teb_amd_obstacles_t t[3] = {two.view(), teb_amd_obstacles_t{}, tri.view()};
    const int32_t vc[3] = {2, 0, 3};
    CHECK(!parse_scene_inputs(3, t, "bad table", vc, vx, vy, roomy, in));
    CHECK(in.rows == 3 && in.verts == 3 && in.vias == 5 && (in.vc == Ints{2, 0, 3}) && in.tabs.size() == 3);
    CHECK(in.tabs[0].rows() == 2 && in.tabs[0].brad[1] == 0.5 && in.tabs[1].rows() == 0 && (in.tabs[1].voff == Ints{0}) && in.tabs[2].verts() == 3);
    // at the limits: accepted; one less of each: refused, rows before vertices before via-points
    CHECK(!parse_scene_inputs(3, t, "bad table", vc, vx, vy, SceneCaps{3, 3, 5}, in));
    CHECK(refused(parse_scene_inputs(3, t, "bad table", vc, vx, vy, SceneCaps{2, 2, 4}, in), TEB_AMD_ERR_CAPACITY, "more obstacles than max_obstacles"));
    CHECK(refused(parse_scene_inputs(3, t, "bad table", vc, vx, vy, SceneCaps{3, 2, 4}, in), TEB_AMD_ERR_CAPACITY, "more polygon vertices than max_obstacle_vertices"));
    CHECK(refused(parse_scene_inputs(3, t, "bad table", vc, vx, vy, SceneCaps{3, 3, 4}, in), TEB_AMD_ERR_CAPACITY, "more via-points than max_via_points"));
    CHECK(!parse_scene_inputs(3, t, "bad table", vc, vx, vy, SceneCaps{}, in));   // no limits: the caller checks later
    // via-points without their arrays: an argument fault, before any capacity
    CHECK(refused(parse_scene_inputs(3, t, "bad table", vc, nullptr, vy, SceneCaps{0, 0, 0}, in), TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays"));
    CHECK(refused(parse_scene_inputs(3, t, "bad table", vc, vx, nullptr, roomy, in), TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays"));
    const int32_t none[3] = {0, 0, 0};
    CHECK(!parse_scene_inputs(3, t, "bad table", none, nullptr, nullptr, roomy, in) && in.vias == 0);
    CHECK(!parse_scene_inputs(3, t, "bad table", nullptr, nullptr, nullptr, roomy, in) && in.vias == 0 && (in.vc == Ints{0, 0, 0}));
  }
  {   // the faults of the scenes in scene order: scene 0's via count before scene 1's table, a table's count before its rows
    teb_amd_obstacles_t neg = bare.view();
    neg.count = -1;
    const teb_amd_obstacles_t t[2] = {two.view(), neg};
    const int32_t bad_first[2] = {-1, 0}, bad_second[2] = {0, -1}, fine[2] = {1, 1};
    CHECK(refused(parse_scene_inputs(2, t, "bad table", bad_first, vx, vy, roomy, in), TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays"));
    CHECK(refused(parse_scene_inputs(2, t, "bad table", bad_second, vx, vy, roomy, in), TEB_AMD_ERR_INVALID_ARG, "bad table"));
    CHECK(refused(parse_scene_inputs(2, t, "null obstacle table", fine, vx, vy, roomy, in), TEB_AMD_ERR_INVALID_ARG, "null obstacle table"));
    const teb_amd_obstacles_t u[2] = {two.view(), bare.view()};
    CHECK(refused(parse_scene_inputs(2, u, "bad table", bad_second, vx, vy, roomy, in), TEB_AMD_ERR_INVALID_ARG, "polygon obstacle without vertex arrays"));
    CHECK(refused(parse_scene_inputs(2, u, "bad table", bad_first, vx, vy, roomy, in), TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays"));
  }
  {   // no tables at all: n empty ones
    CHECK(!parse_scene_inputs(3, nullptr, "bad table", nullptr, nullptr, nullptr, SceneCaps{0, 0, 0}, in));
    CHECK(in.tabs.size() == 3 && in.rows == 0 && in.tabs[2].rows() == 0 && (in.tabs[2].voff == Ints{0}));
  }
  {   // the single scene: one nullable table, no via-points
    CHECK(!parse_scene_inputs(1, nullptr, "bad table", nullptr, nullptr, nullptr, SceneCaps{}, in) && in.tabs.size() == 1 && in.tabs[0].rows() == 0);
    const teb_amd_obstacles_t t = tri.view();
    CHECK(!parse_scene_inputs(1, &t, "bad table", nullptr, nullptr, nullptr, SceneCaps{SIZE_MAX, 3, SIZE_MAX}, in) && in.rows == 1 && in.verts == 3);
    CHECK(refused(parse_scene_inputs(1, &t, "bad table", nullptr, nullptr, nullptr, SceneCaps{SIZE_MAX, 2, SIZE_MAX}, in), TEB_AMD_ERR_CAPACITY,
                  "more polygon vertices than max_obstacle_vertices"));
  }
}

static void check_host_tables() {
  {   // a point, a line, a 6 x 8 rectangle: centroid (3, 4) + (10, 20), bounding radius 5
    const Ints off{0, 1, 3, 7};
    const Reals px{1.5, 2, 4, 10, 16, 16, 10}, py{-1, 2, 6, 20, 20, 28, 28};
    HostObst t;
    CHECK(polygon_list_table(off.data(), px.data(), py.data(), 3, t) == nullptr);
    CHECK((t.type == Ints{TEB_AMD_OBST_POINT, TEB_AMD_OBST_LINE, TEB_AMD_OBST_POLYGON}) && (t.voff == Ints{0, 0, 0, 4}) && (t.dyn == Ints{0, 0, 0}));
    CHECK((t.ax == Reals{1.5, 2, 0}) && (t.ay == Reals{-1, 2, 0}) && (t.bx == Reals{0, 4, 0}) && (t.by == Reals{0, 6, 0}));
    CHECK((t.cx == Reals{1.5, 3, 13}) && (t.cy == Reals{-1, 4, 24}) && (t.rad == Reals{0, 0, 0}));
    CHECK(t.brad[0] == 0.0 && t.brad[1] == 0.5 * std::hypot(2.0, 4.0) && t.brad[2] == 5.0);
    CHECK((t.pvx == Reals{10, 16, 16, 10}) && (t.pvy == Reals{20, 20, 28, 28}));
    const int none[1] = {0};
    CHECK(polygon_list_table(none, nullptr, nullptr, 0, t) == nullptr && t.rows() == 0 && (t.voff == Ints{0}) && t.verts() == 0);
  }
}

// the tables of a set and the out arrays: the last step of the conversion, on rows as the write pass leaves them
static void check_finish() {
  Table circle{{TEB_AMD_OBST_CIRCULAR}, {}, {7}, {8}, {0.25}, {}, {}};
  Table tri{{TEB_AMD_OBST_POLYGON}, {0, 3}, {0}, {0}, {}, {0, 4, 0}, {0, 0, 4}};
  SceneInputs in, bare;
  const teb_amd_obstacles_t custom[3] = {circle.view(), teb_amd_obstacles_t{}, tri.view()};
  CHECK(!parse_scene_inputs(3, custom, "bad table", nullptr, nullptr, nullptr, SceneCaps{}, in));
  CHECK(!parse_scene_inputs(1, nullptr, "bad table", nullptr, nullptr, nullptr, SceneCaps{}, bare));
  std::vector<HostObst> tabs;
  {   // points: scene s holds its tot[s] centres from its prefix on, then its custom rows; as many centres go out as fit
    PointRows K;
    K.rec.resize(3);
    K.tot = {2, 0, 1};
    CHECK(!K.place(in, SceneCaps{}, PointRows::Out{nullptr, nullptr, nullptr, 0}) && K.rows == 3);
    K.px = {1, 2, 3}; K.py = {4, 5, 6};
    for (int cap : {3, 2, 0}) {
      Reals x(4, -1.0), y(4, -1.0);
      CHECK(K.finish(in, PointRows::Out{nullptr, x.data(), y.data(), cap}, tabs) == nullptr);
      CHECK((x == (cap == 3 ? Reals{1, 2, 3, -1} : cap == 2 ? Reals{1, 2, -1, -1} : Reals(4, -1.0))));
      CHECK((y == (cap == 3 ? Reals{4, 5, 6, -1} : cap == 2 ? Reals{4, 5, -1, -1} : Reals(4, -1.0))));
    }
    Reals y(4, -1.0);
    CHECK(K.finish(in, PointRows::Out{nullptr, nullptr, y.data(), 3}, tabs) == nullptr && (y == Reals{4, 5, 6, -1}));   // either array alone
    CHECK(tabs.size() == 3 && (tabs[0].ax == Reals{1, 2, 7}) && (tabs[0].cy == Reals{4, 5, 8}) && (tabs[0].type == Ints{0, 0, TEB_AMD_OBST_CIRCULAR}));
    CHECK((tabs[0].voff == Ints{0, 0, 0, 0}) && (tabs[0].brad == Reals{0, 0, 0.25}));
    CHECK(tabs[1].rows() == 0 && (tabs[1].voff == Ints{0}));
    CHECK((tabs[2].ax == Reals{3, 0}) && (tabs[2].cx[0] == 3) && (tabs[2].voff == Ints{0, 0, 3}) && tabs[2].verts() == 3);
    PointRows E;   // the single scene without a kept cell
    E.rec.resize(1);
    E.tot = {0};
    CHECK(!E.place(bare, SceneCaps{0, 0, 0}, PointRows::Out{nullptr, nullptr, nullptr, 0}));
    CHECK(E.finish(bare, PointRows::Out{nullptr, y.data(), y.data(), 3}, tabs) == nullptr && tabs.size() == 1 && tabs[0].rows() == 0 && (y == Reals{4, 5, 6, -1}));
  }
  const Reals px{1.5, 2, 4, 10, 16, 16, 10}, py{-1, 2, 6, 20, 20, 28, 28};
  {   // polygons: offsets local to each scene's first vertex come back as one list over the whole set; all three out arrays or none
    PolygonRows K;
    K.rec.resize(3);
    K.tot = {2, 0, 1, /* vertices */ 3, 0, 4, /* polygon vertices */ 0, 0, 4};
    const PolygonRows::Out none{nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0};
    auto written = [&](int cap_o, int cap_p, bool with_off, bool with_x, bool with_y) {   // scene 0: a point and a line; scene 2: a polygon
      CHECK(!K.place(in, SceneCaps{}, none) && K.rows == 3 && K.verts == 7 && K.pverts == 4);
      K.off = {0, 1, 0, -1};   // (the terminator is finish's)
      K.px = px; K.py = py;
      Ints o(5, -1);
      Reals x(8, -1.0), y(8, -1.0);
      CHECK(K.finish(in, PolygonRows::Out{nullptr, nullptr, with_off ? o.data() : nullptr, with_x ? x.data() : nullptr, with_y ? y.data() : nullptr, cap_o, cap_p},
                     tabs) == nullptr);
      CHECK((K.off == Ints{0, 1, 3, 7}));
      if (o == Ints(5, -1) && x == Reals(8, -1.0) && y == Reals(8, -1.0)) return false;
      CHECK((o == Ints{0, 1, 3, 7, -1}) && x[6] == 10 && x[7] == -1 && y[6] == 28 && y[7] == -1 && x[0] == 1.5 && y[0] == -1);
      return true;
    };
    CHECK(written(3, 7, true, true, true));     // exactly enough
    CHECK(!written(2, 7, true, true, true));    // one row short
    CHECK(!written(3, 6, true, true, true));    // one vertex short
    CHECK(!written(0, 0, true, true, true));
    CHECK(!written(3, 7, false, true, true) && !written(3, 7, true, false, true) && !written(3, 7, true, true, false));   // an array missing
    CHECK(tabs.size() == 3 && (tabs[0].type == Ints{TEB_AMD_OBST_POINT, TEB_AMD_OBST_LINE, TEB_AMD_OBST_CIRCULAR}) && (tabs[0].bx == Reals{0, 4, 0}));
    CHECK(tabs[1].rows() == 0);
    CHECK((tabs[2].type == Ints{TEB_AMD_OBST_POLYGON, TEB_AMD_OBST_POLYGON}) && (tabs[2].voff == Ints{0, 4, 7}) && tabs[2].cx[0] == 13 && tabs[2].brad[0] == 5.0);
    CHECK((tabs[2].pvx == Reals{10, 16, 16, 10, 0, 4, 0}));
    // the single scene: a set of one, nothing to re-base
    PolygonRows one;
    one.rec.resize(1);
    one.tot = {3, 7, 4};
    CHECK(!one.place(bare, SceneCaps{3, 4, 0}, none));
    one.off = {0, 1, 3, 0};
    one.px = px; one.py = py;
    CHECK(one.finish(bare, none, tabs) == nullptr && (one.off == Ints{0, 1, 3, 7}) && tabs[0].rows() == 3 && (tabs[0].voff == Ints{0, 0, 0, 4}));
    // no rows at all: the empty list is its terminator, and fits capacities of 0
    PolygonRows empty;
    empty.rec.resize(1);
    empty.tot = {0, 0, 0};
    CHECK(!empty.place(bare, SceneCaps{0, 0, 0}, none) && (empty.off == Ints{0}));
    Ints e(2, -1);
    Reals x(1, -1.0), y(1, -1.0);
    CHECK(empty.finish(bare, PolygonRows::Out{nullptr, nullptr, e.data(), x.data(), y.data(), 0, 0}, tabs) == nullptr);
    CHECK((e == Ints{0, -1}) && x[0] == -1.0 && tabs.size() == 1 && tabs[0].rows() == 0);
  }
}

int main() {
  check_lane_rule();
  check_block_geometry();
  check_filter();
  check_set_layout();
  check_input_parse();
  check_host_tables();
  check_finish();
  if (g_failures == 0) std::printf("costmap host check ok\n");
  return g_failures;
}
