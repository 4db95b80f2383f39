// teb_scene_store.hpp — ONE obstacle table, host side and device side, for the single scene of a handle and for a scene set (fleet
// batches, teb_fleet.hpp) alike. The host part (HostObst, its parse, the lists derived from it, the segments of a scene set) is plain
// C++ over include/teb_amd.h: tests/host/scene_table_check.cpp compiles it alone with -DTEB_SCENE_STORE_HOST_ONLY. So is DevBuf, the
// owner of every device allocation of the library, over two primitives its includer defines. The device part (DevSceneStore) needs the
// HIP runtime and SceneDev.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>
#ifndef TEB_SCENE_STORE_HOST_ONLY
#include <hip/hip_runtime.h>
#endif

#include "../../include/teb_amd.h"

namespace tebamd {

// ---- device memory that owns itself -----------------------------------------------------------------------------------------------
// The two primitives every DevBuf goes through, DEFINED BY THE INCLUDER: teb_amd.hip with hipMalloc / hipFree, the host check
// (tests/host/band_store_check.cpp) with counters. DevError is hipError_t, or int without HIP; 0 is success (hipSuccess) in both.
#ifdef TEB_SCENE_STORE_HOST_ONLY
using DevError = int;
#else
using DevError = hipError_t;
#endif
constexpr DevError kDevOk = DevError{};
DevError device_allocate(void** p, size_t bytes);
void device_free(void* p);

// `count` elements of device memory, owned: freed by the destructor, by free(), by an alloc() over it and by a move onto it. Move-only,
// so nothing frees a buffer twice. No DevBuf may have static storage duration: its destructor would run after the runtime's own teardown.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { free(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
    return *this;
  }
  ~DevBuf() { free(); }
  // (count 0: one element, so that p is an address; a failure leaves the buffer empty)
  DevError alloc(size_t count) {
    free();
    void* q = nullptr;
    const DevError e = device_allocate(&q, (count ? count : 1) * sizeof(T));
    if (e == kDevOk) { p = static_cast<T*>(q); n = count; }
    return e;
  }
  void free() {
    if (p) device_free(p);
    p = nullptr; n = 0;
  }
};
// scratch that only grows: b holds at least count elements afterwards (its contents are lost when it grows)
template <typename T>
DevError ensure(DevBuf<T>& b, size_t count) {
  return b.n >= count ? kDevOk : b.alloc(count);
}
// A run of allocations that belong together: A(buf.alloc(..)) for each, then ok() / first (the first failure). What to do about a
// failure - free the set, fail the call - is the caller's.
struct AllocRun {
  DevError first = kDevOk;
  void operator()(DevError e) { if (first == kDevOk) first = e; }
  bool ok() const { return first == kDevOk; }
};

// How long a column of an obstacle table is: one entry per row, one per row + 1 (first-vertex offsets), one per polygon vertex.
enum class ColumnExtent { Rows, Voff, Verts };

// THE column enumeration: f(column of a, the same column of b, its extent) for the 13 row columns and the 2 vertex columns. a and b are
// any two of HostObst / DevSceneStore (they name their columns alike); pass the same object twice to visit one table.
template <class A, class B, class F>
void for_each_column(A& a, B& b, F&& f) {
  f(a.type, b.type, ColumnExtent::Rows); f(a.dyn, b.dyn, ColumnExtent::Rows); f(a.voff, b.voff, ColumnExtent::Voff);
  f(a.ax, b.ax, ColumnExtent::Rows); f(a.ay, b.ay, ColumnExtent::Rows); f(a.bx, b.bx, ColumnExtent::Rows); f(a.by, b.by, ColumnExtent::Rows);
  f(a.rad, b.rad, ColumnExtent::Rows); f(a.vx, b.vx, ColumnExtent::Rows); f(a.vy, b.vy, ColumnExtent::Rows);
  f(a.cx, b.cx, ColumnExtent::Rows); f(a.cy, b.cy, ColumnExtent::Rows); f(a.brad, b.brad, ColumnExtent::Rows);
  f(a.pvx, b.pvx, ColumnExtent::Verts); f(a.pvy, b.pvy, ColumnExtent::Verts);
}

// Host copy of an obstacle table (teb_amd_obstacles_t) with the centroids and bounding radii the kernels read. voff holds rows() + 1
// first-vertex offsets into pvx / pvy, starting at 0.
struct HostObst {
  std::vector<int> type, dyn, voff;
  std::vector<double> ax, ay, bx, by, rad, vx, vy, cx, cy, brad, pvx, pvy;

  size_t rows() const { return type.size(); }
  size_t verts() const { return pvx.size(); }
  // n zeroed rows without vertices
  void reset_rows(size_t n) {
    for_each_column(*this, *this, [n](auto& c, auto&, ColumnExtent e) { c.assign(e == ColumnExtent::Rows ? n : e == ColumnExtent::Voff ? n + 1 : 0, 0); });
  }
  // o behind this table as a SEGMENT of its own: every column one after the other, o's rows() + 1 offsets still local to o's vertices
  // (the layout of a scene set: scene_segments)
  void append_segment(const HostObst& o) {
    for_each_column(*this, o, [](auto& d, const auto& s, ColumnExtent) { d.insert(d.end(), s.begin(), s.end()); });
  }
  // o behind this table as further rows of ONE table: o's offsets move by the vertices already held. Both tables hold their
  // rows() + 1 offsets (parse_obstacle_table, reset_rows).
  void append(const HostObst& o) {
    const int shift = (int)verts();
    const size_t at = rows();
    voff.pop_back();   // (its terminator is o's first offset)
    append_segment(o);
    for (size_t i = at; i < voff.size(); ++i) voff[i] += shift;
  }
};

// PolygonObstacle::calcCentroid (reference src/obstacles.cpp:56-121) — product-side implementation
inline void polygon_centroid(const double* vx, const double* vy, int n, double& cx, double& cy) {
  if (n <= 0) { cx = cy = std::numeric_limits<double>::quiet_NaN(); return; }
  if (n == 1) { cx = vx[0]; cy = vy[0]; return; }
  if (n == 2) { cx = 0.5 * (vx[0] + vx[1]); cy = 0.5 * (vy[0] + vy[1]); return; }
  double A = 0;
  for (int i = 0; i < n - 1; ++i) A += vx[i] * vy[i + 1] - vx[i + 1] * vy[i];
  A += vx[n - 1] * vy[0] - vx[0] * vy[n - 1];
  A *= 0.5;
  if (A != 0) {
    cx = 0; cy = 0;
    for (int i = 0; i < n - 1; ++i) {
      double aux = vx[i] * vy[i + 1] - vx[i + 1] * vy[i];
      cx += (vx[i] + vx[i + 1]) * aux;
      cy += (vy[i] + vy[i + 1]) * aux;
    }
    double aux = vx[n - 1] * vy[0] - vx[0] * vy[n - 1];
    cx += (vx[n - 1] + vx[0]) * aux;
    cy += (vy[n - 1] + vy[0]) * aux;
    cx /= (6 * A);
    cy /= (6 * A);
    return;
  }
  int ic = 0, jc = 0;
  double md = 0;
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      double d = std::sqrt((vx[j] - vx[i]) * (vx[j] - vx[i]) + (vy[j] - vy[i]) * (vy[j] - vy[i]));
      if (d > md) { md = d; ic = i; jc = j; }
    }
  cx = 0.5 * (vx[ic] + vx[jc]);
  cy = 0.5 * (vy[ic] + vy[jc]);
}

// The host side of an obstacle table with the centroids and bounding radii the kernels read; t.voff and the vertices start at 0.
// Checks the arrays, not the capacities. Returns null, or what is wrong with the table (an invalid argument of the caller's).
inline const char* parse_obstacle_table(const teb_amd_obstacles_t* o, HostObst& t) {
  const int M = o->count;
  if (M > 0 && (!o->type || !o->ax || !o->ay)) return "obstacle arrays missing";
  t.reset_rows(M);
  for (int i = 0; i < M; ++i) {
    t.type[i] = o->type[i];
    t.ax[i] = o->ax[i]; t.ay[i] = o->ay[i];
    t.bx[i] = o->bx ? o->bx[i] : 0; t.by[i] = o->by ? o->by[i] : 0;
    t.rad[i] = o->radius ? o->radius[i] : 0;
    t.vx[i] = o->vx ? o->vx[i] : 0; t.vy[i] = o->vy ? o->vy[i] : 0;
    t.dyn[i] = o->dynamic ? (o->dynamic[i] != 0) : 0;
    t.voff[i] = (int)t.pvx.size();
    switch (t.type[i]) {
      case TEB_AMD_OBST_POINT: case TEB_AMD_OBST_CIRCULAR: t.cx[i] = t.ax[i]; t.cy[i] = t.ay[i]; t.brad[i] = std::fabs(t.rad[i]); break;
      case TEB_AMD_OBST_LINE: case TEB_AMD_OBST_PILL:
        t.cx[i] = 0.5 * (t.ax[i] + t.bx[i]); t.cy[i] = 0.5 * (t.ay[i] + t.by[i]);
        t.brad[i] = 0.5 * std::hypot(t.bx[i] - t.ax[i], t.by[i] - t.ay[i]) + std::fabs(t.rad[i]);
        break;
      case TEB_AMD_OBST_POLYGON: {
        if (!o->vert_offset || !o->vert_x || !o->vert_y) return "polygon obstacle without vertex arrays";
        int k0 = o->vert_offset[i], k1 = o->vert_offset[i + 1];
        if (k1 <= k0) return "polygon obstacle without vertices";
        for (int k = k0; k < k1; ++k) { t.pvx.push_back(o->vert_x[k]); t.pvy.push_back(o->vert_y[k]); }
        polygon_centroid(o->vert_x + k0, o->vert_y + k0, k1 - k0, t.cx[i], t.cy[i]);
        for (int k = k0; k < k1; ++k) t.brad[i] = std::max(t.brad[i], std::hypot(o->vert_x[k] - t.cx[i], o->vert_y[k] - t.cy[i]));
        if (!(t.brad[i] == t.brad[i])) t.brad[i] = std::numeric_limits<double>::infinity();   // NaN centroid: never culled
        break;
      }
      default: return "unknown obstacle type";
    }
  }
  t.voff[M] = (int)t.pvx.size();
  return nullptr;
}

// What ONE scene's kernels read beyond the rows of its table, derived from the table and the configuration: the lists
// AddEdgesObstacles / AddEdgesDynamicObstacles visit, the obstacles in cache order, static_radius_zero, point-likeness.
struct SceneLists {
  std::vector<int> st, dy;
  std::vector<double> lo;        // [5][rows]: x, y, radius, vx, vy in cache order (static list, then dynamic list)
  int static_radius_zero = 1;    // no circular obstacle with a radius in the static list
  bool pointlike_rows = true;    // every row is Point / Circular
};
inline void derive_scene_lists(const teb_amd_config_t& cfg, const HostObst& o, SceneLists& d) {
  const size_t stride = o.rows();
  const int M = (int)stride;
  d.st.clear(); d.dy.clear();
  d.pointlike_rows = true;
  for (int i = 0; i < M; ++i) {
    d.pointlike_rows = d.pointlike_rows && (o.type[i] == TEB_AMD_OBST_POINT || o.type[i] == TEB_AMD_OBST_CIRCULAR);
    // AddEdgesObstacles skips dynamic obstacles iff include_dynamic_obstacles (optimal_planner.cpp:496-497);
    // AddEdgesDynamicObstacles visits the dynamic ones (:658-659)
    if (cfg.include_dynamic_obstacles && o.dyn[i]) d.dy.push_back(i); else d.st.push_back(i);
  }
  // the obstacles in cache order (static list, then dynamic list): what the kernel stages into LDS, readable with scalar loads
  d.lo.assign(5 * stride, 0.0);
  size_t k = 0;
  d.static_radius_zero = 1;
  for (int oi : d.st) if (o.type[oi] == TEB_AMD_OBST_CIRCULAR && o.rad[oi] != 0.0) d.static_radius_zero = 0;
  for (const std::vector<int>* lst : {&d.st, &d.dy})
    for (int oi : *lst) {
      d.lo[k] = o.ax[oi]; d.lo[stride + k] = o.ay[oi]; d.lo[2 * stride + k] = o.type[oi] == TEB_AMD_OBST_CIRCULAR ? o.rad[oi] : 0.0;
      d.lo[3 * stride + k] = o.vx[oi]; d.lo[4 * stride + k] = o.vy[oi];
      ++k;
    }
}

// Where scene s of a scene set starts in the columns of its store: the scenes lie one after the other (HostObst::append_segment), a
// scene of M rows takes M rows, M + 1 offsets, its vertices, its via-points and 5 M entries of the cache list (planes of stride M).
struct SceneSegment { size_t row = 0, voff = 0, vert = 0, via = 0, list = 0; };
inline std::vector<SceneSegment> scene_segments(const HostObst* tabs, const int* via_count, size_t n_scenes) {
  std::vector<SceneSegment> seg(n_scenes);
  size_t ro = 0, vo = 0, wo = 0;
  for (size_t s = 0; s < n_scenes; ++s) {
    seg[s].row = ro; seg[s].voff = ro + s; seg[s].vert = vo; seg[s].via = wo; seg[s].list = 5 * ro;
    ro += tabs[s].rows(); vo += tabs[s].verts(); wo += (size_t)via_count[s];
  }
  return seg;
}

}  // namespace tebamd

#ifndef TEB_SCENE_STORE_HOST_ONLY
#include "teb_device.hpp"
#include "teb_costmap_pods.hpp"   // CmoRows

namespace tebamd {

// count elements to the device on the stream (none: nothing enqueued); src is read until the stream is synchronised
template <typename T>
hipError_t upload(hipStream_t stream, T* dst, const T* src, size_t count) {
  return count == 0 ? hipSuccess : hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, stream);
}

// The device side of one or several obstacle tables: the columns of HostObst, the lists derived from them (SceneLists) and the
// via-points. A handle owns two: the store of its single scene and, from the first teb_amd_set_scenes on, the store of the scene set.
struct DevSceneStore {
  DevBuf<int> type, dyn, voff;
  DevBuf<double> ax, ay, bx, by, rad, vx, vy, cx, cy, brad, pvx, pvy;
  DevBuf<int> stat, dynidx;   // SceneDev::static_idx, dyn_idx
  DevBuf<double> list;        // [5][M] per scene: x, y, radius, vx, vy in the order of the LDS obstacle cache (SceneDev::lox ..)
  DevBuf<double> viax, viay;

  // rows / verts / vias: capacities; voff_extra: offsets beyond one per row (1 for a table, one per scene for a scene set); pad:
  // elements past every buffer, so that the segment of an empty scene at the very end still points at storage
  bool alloc(size_t rows, size_t voff_extra, size_t verts, size_t vias, size_t pad) {
    AllocRun A;
    rows += pad;
    for_each_column(*this, *this, [&](auto& c, auto&, ColumnExtent e) {
      A(c.alloc(e == ColumnExtent::Rows ? rows : e == ColumnExtent::Voff ? rows + voff_extra : verts + pad));
    });
    A(stat.alloc(rows)); A(dynidx.alloc(rows)); A(list.alloc(5 * rows)); A(viax.alloc(vias + pad)); A(viay.alloc(vias + pad));
    return A.ok();
  }
  // Enqueues the columns of t: rows from first_row on, its offsets from first_voff on, its vertices from first_vert on. The copies
  // read t until the stream is synchronised.
  hipError_t upload_rows(hipStream_t stream, const HostObst& t, size_t first_row, size_t first_voff, size_t first_vert) {
    hipError_t err = hipSuccess;
    for_each_column(*this, t, [&](auto& d, const auto& v, ColumnExtent e) {
      const size_t first = e == ColumnExtent::Rows ? first_row : e == ColumnExtent::Voff ? first_voff : first_vert;
      if (err == hipSuccess) err = upload(stream, d.p + first, v.data(), v.size());
    });
    return err;
  }
  hipError_t upload_vias(hipStream_t stream, const double* x, const double* y, size_t count) {
    const hipError_t err = upload(stream, viax.p, x, count);
    return err != hipSuccess ? err : upload(stream, viay.p, y, count);
  }
  // Enqueues the lists of every scene, each at its segment: st / dy one entry per row, lo five (read until the stream is synchronised).
  hipError_t upload_lists(hipStream_t stream, const SceneLists& all) {
    hipError_t err = upload(stream, stat.p, all.st.data(), all.st.size());
    if (err == hipSuccess) err = upload(stream, dynidx.p, all.dy.data(), all.dy.size());
    return err != hipSuccess ? err : upload(stream, list.p, all.lo.data(), all.lo.size());
  }
  // The pointer part of the SceneDev of the scene at segment g with M rows (its indices are local to the segment, so the kernel's
  // arithmetic does not know about segments); n_static, n_dyn, static_radius_zero: of the lists upload_lists put there.
  SceneDev view(const SceneSegment& g, int M, int nvia, int n_static, int n_dyn, int static_radius_zero, int fast_points) const {
    SceneDev s;
    s.M = M;
    s.fast_points = fast_points;
    s.static_radius_zero = static_radius_zero;
    s.type = type.p + g.row; s.ax = ax.p + g.row; s.ay = ay.p + g.row; s.bx = bx.p + g.row; s.by = by.p + g.row;
    s.rad = rad.p + g.row; s.vx = vx.p + g.row; s.vy = vy.p + g.row; s.cx = cx.p + g.row; s.cy = cy.p + g.row; s.brad = brad.p + g.row;
    s.dyn = dyn.p + g.row; s.voff = voff.p + g.voff; s.pvx = pvx.p + g.vert; s.pvy = pvy.p + g.vert;
    s.n_static = n_static; s.static_idx = stat.p + g.row; s.n_dyn = n_dyn; s.dyn_idx = dynidx.p + g.row;
    s.nvia = nvia; s.viax = viax.p + g.via; s.viay = viay.p + g.via;
    s.lox = list.p + g.list; s.loy = s.lox + M; s.lor = s.lox + 2 * (size_t)M; s.lovx = s.lox + 3 * (size_t)M; s.lovy = s.lox + 4 * (size_t)M;
    return s;
  }
  // the rows the costmap writer fills (costmap_obstacles_write_kernel, teb_costmap_obstacles.hpp)
  CmoRows rows() const { return CmoRows{type.p, dyn.p, voff.p, ax.p, ay.p, bx.p, by.p, rad.p, vx.p, vy.p, cx.p, cy.p, brad.p}; }
};

}  // namespace tebamd
#endif  // TEB_SCENE_STORE_HOST_ONLY
