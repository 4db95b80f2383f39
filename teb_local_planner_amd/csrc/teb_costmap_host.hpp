// teb_costmap_host.hpp — a costmap becomes an obstacle table: the host rules of that conversion, each stated once for its two row kinds
// (one point per lethal cell, teb_costmap_obstacles.hpp; convex polygons per tile, teb_costmap_polygons.hpp) and its two routes (the
// single scene of a handle, the scenes of a set): the launch geometry, the place of every scene of a set in the shared scratch, the
// parse of the caller's tables and via-points, the host tables and the out-array rules. Plain C++ over include/teb_amd.h,
// teb_costmap_pods.hpp (what the kernels read) and the host part of teb_scene_store.hpp: tests/host/costmap_host_check.cpp compiles it
// alone with -DTEB_SCENE_STORE_HOST_ONLY. The launches, copies and synchronisations are the driver's (teb_amd.hip, convert_costmaps).
#pragma once

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "teb_costmap_pods.hpp"
#include "teb_scene_store.hpp"

namespace tebamd {

// Why a call is refused: the return code and the text of teb_amd_last_error (a literal, or the parse's). code 0: not refused.
struct Refusal {
  int code = TEB_AMD_OK;
  const char* text = nullptr;
  explicit operator bool() const { return code != TEB_AMD_OK; }
};

inline CmoFilter costmap_filter(const double* pose, double behind_robot_dist) {
  return CmoFilter{pose[0], pose[1], std::cos(pose[2]), std::sin(pose[2]), behind_robot_dist};
}

// ---- launch geometry -----------------------------------------------------------------------------------------------------------------
// The lanes of the point route over a grid: one per (column, chunk of rows) of the visit domain (sx - 1) x (sy - 1). Rows per lane: the
// smallest of 4, 8, .. 64 that keeps the lanes (= values to scan) within 64 K - a 120 x 120 grid gets 4 rows per lane (3570 lanes, 56
// waves), a 1000 x 1000 grid 16 (62937 lanes); from 4096 x 4096 on the chunk stays 64 and the lanes grow.
struct CmoLanes {
  int ncols, nrows, chunk, nchunks;
  size_t lanes() const { return (size_t)ncols * nchunks; }
};
inline CmoLanes point_lanes(int size_x, int size_y) {
  CmoLanes l{size_x - 1, size_y - 1, 4, 0};
  if (l.ncols <= 0 || l.nrows <= 0) return CmoLanes{0, 0, 4, 0};
  while (l.chunk < 64 && (size_t)l.ncols * (size_t)((l.nrows + l.chunk - 1) / l.chunk) > 65536) l.chunk *= 2;
  l.nchunks = (l.nrows + l.chunk - 1) / l.chunk;
  return l;
}

// The blocks of the polygon route over a grid at tile size T (1 .. kCmpMaxTile): q and the number of blocks (0: no visit domain), or
// -1 for a grid of more than 2^30 blocks ("grid too large").
inline long long polygon_blocks(int size_x, int size_y, int T, CmpGeom& q) {
  q = CmpGeom{size_x - 1, size_y - 1, T, kCmpSlots / (T * T), 0, 0};
  if (q.ncols <= 0 || q.nrows <= 0) return 0;
  q.nty = (q.nrows + T - 1) / T;
  q.nby = (q.nty + q.k - 1) / q.k;
  const long long nb = (long long)((q.ncols + T - 1) / T) * q.nby;
  return nb > (1 << 30) ? -1 : nb;
}

// ---- what the caller hands in -------------------------------------------------------------------------------------------------------
// The obstacle tables of n scenes (teb_amd_set_obstacles' parse: same centroids, radii, vertex offsets from 0) and their via counts.
struct SceneInputs {
  std::vector<HostObst> tabs;
  std::vector<int> vc;
  size_t rows = 0, verts = 0, vias = 0;
};
// What tables and via-points may hold together: the handle's capacities. The parse refuses at them (SIZE_MAX: not here - the caller
// checks that sum later, together with what it converts).
struct SceneCaps { size_t rows = SIZE_MAX, verts = SIZE_MAX, vias = SIZE_MAX; };
// tables: n tables, or null for n empty ones; bad_count: the text for a negative count; via_count: null for no via-points.
// Everything is parsed and checked before the caller's first launch or upload: the first fault, in this order, is the refusal.
inline Refusal parse_scene_inputs(int n, const teb_amd_obstacles_t* tables, const char* bad_count, const int32_t* via_count, const double* via_x,
                                  const double* via_y, const SceneCaps& cap, SceneInputs& in) {
  in = SceneInputs{};
  in.tabs.resize(n);
  in.vc.assign(n, 0);
  const teb_amd_obstacles_t none{};
  for (int s = 0; s < n; ++s) {
    if (tables && tables[s].count < 0) return Refusal{TEB_AMD_ERR_INVALID_ARG, bad_count};
    if (const char* bad = parse_obstacle_table(tables ? &tables[s] : &none, in.tabs[s])) return Refusal{TEB_AMD_ERR_INVALID_ARG, bad};
    in.rows += in.tabs[s].rows(); in.verts += in.tabs[s].verts();
    if (via_count) {
      if (via_count[s] < 0) return Refusal{TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays"};
      in.vc[s] = via_count[s]; in.vias += (size_t)via_count[s];
    }
  }
  if (in.vias > 0 && (!via_x || !via_y)) return Refusal{TEB_AMD_ERR_INVALID_ARG, "bad via-point arrays"};
  if (in.rows > cap.rows) return Refusal{TEB_AMD_ERR_CAPACITY, "more obstacles than max_obstacles"};
  if (in.verts > cap.verts) return Refusal{TEB_AMD_ERR_CAPACITY, "more polygon vertices than max_obstacle_vertices"};
  if (in.vias > cap.vias) return Refusal{TEB_AMD_ERR_CAPACITY, "more via-points than max_via_points"};
  return Refusal{};
}

// ---- host tables: exactly what teb_amd_set_obstacles / teb_amd_set_scenes would hold ---------------------------------------------------
// n points: radius 0, velocity 0, not dynamic, no vertices
inline HostObst point_rows_table(const double* x, const double* y, size_t n) {
  static_assert(TEB_AMD_OBST_POINT == 0, "zeroed rows are point rows");
  HostObst t;
  t.reset_rows(n);
  std::copy(x, x + n, t.ax.begin());
  std::copy(y, y + n, t.ay.begin());
  t.cx = t.ax; t.cy = t.ay;
  return t;
}

// A polygon list (row i has the vertices off[i] .. off[i + 1] - 1 of px / py) as an obstacle table: 1 vertex a point, 2 a line, more a
// polygon; radius 0, velocity 0, not dynamic. Through teb_amd_set_obstacles' parse, so that centroids and bounding radii are the same
// code. Returns null or what is wrong.
inline const char* polygon_list_table(const int* off, const double* px, const double* py, int nr, HostObst& t) {
  std::vector<int> type(nr), voff(nr + 1, 0);
  std::vector<double> ax(nr), ay(nr), bx(nr, 0.0), by(nr, 0.0), pgx, pgy;
  for (int i = 0; i < nr; ++i) {
    const int k0 = off[i], k = off[i + 1] - k0;
    type[i] = k == 1 ? TEB_AMD_OBST_POINT : k == 2 ? TEB_AMD_OBST_LINE : TEB_AMD_OBST_POLYGON;
    ax[i] = k <= 2 ? px[k0] : 0.0; ay[i] = k <= 2 ? py[k0] : 0.0;   // a polygon is its vertices (ObstacleTable.add_polygon)
    if (k == 2) { bx[i] = px[k0 + 1]; by[i] = py[k0 + 1]; }
    if (k >= 3) { pgx.insert(pgx.end(), px + k0, px + k0 + k); pgy.insert(pgy.end(), py + k0, py + k0 + k); }
    voff[i + 1] = (int)pgx.size();
  }
  teb_amd_obstacles_t ct{};
  ct.count = nr; ct.type = type.data(); ct.ax = ax.data(); ct.ay = ay.data(); ct.bx = bx.data(); ct.by = by.data();
  ct.vert_offset = voff.data(); ct.vert_x = pgx.data(); ct.vert_y = pgy.data();
  return parse_obstacle_table(&ct, t);
}

// ---- the two row kinds. Each holds the records of the scenes of a set (the single scene: a set of one), their totals and the
// converted rows, and states three steps of the conversion: layout (the launch geometry per grid and the place of every scene in the
// shared scratch, before the count pass), place (after it: counts reported, prefixes set, refused if the rows would not fit) and
// finish (after the write pass: every scene's converted rows ++ its custom rows as host tables, and the out arrays) ---------------------
// Points: one row per kept cell. A scene has lanes + 1 counters, the scenes one after the other.
struct PointRows {
  struct Out { int32_t* n_costmap; double *x, *y; int capacity; };
  std::vector<CmoSceneRec> rec;
  size_t counters = 0, max_lanes = 0;   // counters of the set; the most lanes of a scene
  std::vector<int> tot;                 // kept cells per scene
  size_t rows = 0;                      // of the set
  std::vector<double> px, py;           // the centres of the set, scene s from rec[s].out_off on

  Refusal layout(const GridDev* grids, int n, const double* poses, double behind_robot_dist, const int32_t* /* tiles */) {
    rec.resize(n);
    tot.assign(n, 0);
    for (int s = 0; s < n; ++s) {
      const CmoLanes l = point_lanes(grids[s].sx, grids[s].sy);
      rec[s] = CmoSceneRec{grids[s], costmap_filter(poses + 3 * (size_t)s, behind_robot_dist), l.ncols, l.nrows, l.chunk, l.nchunks, (int)counters, 0};
      counters += l.lanes() + 1;
      max_lanes = std::max(max_lanes, l.lanes());
      if (counters > (size_t)INT_MAX) return Refusal{TEB_AMD_ERR_CAPACITY, "the grids of the set are too large for one call"};
    }
    return Refusal{};
  }
  // (the prefixes saturate: a sum they cannot hold is refused here, before any launch reads them)
  Refusal place(const SceneInputs& in, const SceneCaps& cap, const Out& o) {
    rows = 0;
    for (size_t s = 0; s < rec.size(); ++s) {
      rec[s].out_off = (int)std::min<size_t>(rows, (size_t)INT_MAX);
      rows += (size_t)tot[s];
    }
    if (o.n_costmap) std::copy(tot.begin(), tot.end(), o.n_costmap);
    if (rows + in.rows > cap.rows) return Refusal{TEB_AMD_ERR_CAPACITY, "costmap cells + custom obstacles exceed max_obstacles"};
    px.resize(rows); py.resize(rows);
    return Refusal{};
  }
  // out arrays: as many centres as fit
  const char* finish(const SceneInputs& in, const Out& o, std::vector<HostObst>& tabs) {
    tabs.resize(rec.size());
    for (size_t s = 0; s < rec.size(); ++s) {
      tabs[s] = point_rows_table(px.data() + rec[s].out_off, py.data() + rec[s].out_off, (size_t)tot[s]);
      tabs[s].append(in.tabs[s]);
    }
    const size_t give = std::min((size_t)o.capacity, rows);
    if (o.x) std::copy(px.begin(), px.begin() + give, o.x);
    if (o.y) std::copy(py.begin(), py.begin() + give, o.y);
    return nullptr;
  }
};

// Polygons: one row per 8-connected component of a tile. The blocks of the scenes form one flat list (blk0: n + 1 prefix entries, what
// the kernels search their scene in; a scene without blocks shares its entry with the next); a scene has nblk + 1 counters in each of
// three arrays (rows, vertices, polygon vertices) of ncnt.
struct PolygonRows {
  struct Out { int32_t *n_obstacles, *n_points, *offset; double *x, *y; int capacity_obstacles, capacity_points; };
  std::vector<CmpSceneRec> rec;
  std::vector<int> blk0;
  long long blocks = 0, ncnt = 0;
  std::vector<int> tot;                      // [rows | vertices | polygon vertices][scene]
  long long rows = 0, verts = 0, pverts = 0; // of the set
  // the polygon list of the set: rows + 1 first-vertex offsets into px / py. From the write pass scene s has its offsets from
  // rec[s].row0 on, counted from its first vertex rec[s].vtx0; finish makes them one list
  std::vector<int> off;
  std::vector<double> px, py;

  Refusal layout(const GridDev* grids, int n, const double* poses, double behind_robot_dist, const int32_t* tiles) {
    rec.resize(n);
    blk0.assign((size_t)n + 1, 0);
    tot.assign(3 * (size_t)n, 0);
    for (int s = 0; s < n; ++s) {
      CmpSceneRec& r = rec[s];
      const long long nb = polygon_blocks(grids[s].sx, grids[s].sy, tiles[s], r.q);
      if (nb < 0) return Refusal{TEB_AMD_ERR_CAPACITY, "grid too large"};
      r.g = grids[s];
      r.f = costmap_filter(poses + 3 * (size_t)s, behind_robot_dist);
      r.blk0 = blk0[s] = (int)blocks; r.nblk = (int)nb; r.cnt0 = (int)ncnt; r.row0 = 0; r.vtx0 = 0;
      blocks += nb; ncnt += nb + 1;
      if (blocks > INT_MAX || 3 * ncnt > INT_MAX) return Refusal{TEB_AMD_ERR_CAPACITY, "the grids of the set are too large for one call"};
    }
    blk0[n] = (int)blocks;
    return Refusal{};
  }
  Refusal place(const SceneInputs& in, const SceneCaps& cap, const Out& o) {
    const size_t n = rec.size();
    rows = verts = pverts = 0;
    for (size_t s = 0; s < n; ++s) {
      rec[s].row0 = (int)std::min<long long>(rows, INT_MAX); rec[s].vtx0 = (int)std::min<long long>(verts, INT_MAX);
      rows += tot[s]; verts += tot[n + s]; pverts += tot[2 * n + s];
    }
    if (o.n_obstacles) std::copy(tot.begin(), tot.begin() + n, o.n_obstacles);
    if (o.n_points) std::copy(tot.begin() + n, tot.begin() + 2 * n, o.n_points);
    if ((size_t)rows + in.rows > cap.rows) return Refusal{TEB_AMD_ERR_CAPACITY, "converted costmap rows + custom obstacles exceed max_obstacles"};
    if ((size_t)pverts + in.verts > cap.verts) return Refusal{TEB_AMD_ERR_CAPACITY, "more polygon vertices than max_obstacle_vertices"};
    // (rows <= max_obstacles; a point or line row has at most 2 vertices: verts <= 2 max_obstacles + max_obstacle_vertices)
    off.assign((size_t)rows + 1, 0);
    px.resize((size_t)verts); py.resize((size_t)verts);
    return Refusal{};
  }
  // off becomes the list of the whole set: re-based to the set's first vertex, closed by its vertices; a scene's rows are a stretch
  // of it. Out arrays: all three or none, and only when both capacities suffice.
  const char* finish(const SceneInputs& in, const Out& o, std::vector<HostObst>& tabs) {
    const size_t n = rec.size();
    tabs.assign(n, HostObst{});
    for (size_t s = 0; s < n; ++s)
      for (int i = 0; i < tot[s]; ++i) off[(size_t)rec[s].row0 + i] += rec[s].vtx0;
    off.back() = (int)verts;
    for (size_t s = 0; s < n; ++s) {
      if (const char* bad = polygon_list_table(off.data() + rec[s].row0, px.data(), py.data(), tot[s], tabs[s])) return bad;
      tabs[s].append(in.tabs[s]);
    }
    if (o.offset && o.x && o.y && rows <= o.capacity_obstacles && verts <= o.capacity_points) {
      std::copy(off.begin(), off.end(), o.offset);
      std::copy(px.begin(), px.end(), o.x);
      std::copy(py.begin(), py.end(), o.y);
    }
    return nullptr;
  }
};

}  // namespace tebamd
