// teb_costmap_polygons.hpp — the costmap's lethal cells as a few convex obstacles, built on the device: what a costmap converter plugin
// hands TebLocalPlannerROS::updateObstacleContainerWithCostmapConverter (src/teb_local_planner_ros.cpp:506-549), under the rule of
// include/teb_amd.h (teb_amd_set_obstacles_from_costmap_polygons):
//   kept cells  : costmap_point_obstacle (teb_costmap_obstacles.hpp) - the cells the point route keeps;
//   tiles       : T x T cells anchored at cell (0, 0), clipped to the visit domain;
//   components  : 8-connected kept cells of one tile;
//   row         : the convex hull of a component's cell indices (Andrew's monotone chain on integers, strict turns only) - 1 vertex a
//                 point, 2 a line from the lexicographically smallest to the largest (mx, my), more a counter-clockwise polygon from
//                 the smallest vertex on;
//   order       : tiles tx outer, ty inner; inside a tile by the smallest (mx, my) cell of the component.
//
// A workgroup owns a BLOCK: the tiles (tx, ty0 .. ty0 + k - 1) of one tile column, k = kCmpSlots / T^2 (one 64 x 64 tile, 64 tiles of
// 8 x 8, 4096 tiles of one cell). Blocks in (tx, ty0) order are table order, so a scan over blocks gives every row its place. Every
// cell of a block has a slot in LDS, slot = j * T^2 + dx * T + ddy (tile j of the block, column dx and row ddy inside the tile): slot
// order is table order, and the smallest slot of a component is its smallest (mx, my). cmp_block (below) works a block out:
//   1. kept mask: lab[slot] = slot for a kept cell, -1 otherwise;
//   2. components: union-find over the in-tile neighbours (dx + 1, ddy - 1 .. ddy + 1) and (dx, ddy + 1), linking a root under a
//      smaller one with atomicMin and halving paths on the way, then every label compressed to its root. The root of a component is
//      its smallest slot whatever the schedule, so labels are canonical; the work is near linear in the cells, whatever their shape;
//   3. per component its last column (the columns of an 8-connected set are contiguous, the first is the root's); one scan over the
//      slots gives each component its row rank in the block and a segment of (columns) entries for the lowest and highest cell of each
//      column - the hull candidates, sorted by mx as the monotone chain wants them;
//   4. one lane per component: the lower chain over the column minima and the upper chain over the column maxima, each in place in its
//      own segment; with the two shared end points dropped where they coincide this is exactly Andrew's chain over all the candidates
//      (a column's maximum never survives the lower chain but at the last column, nor its minimum the upper chain but at the first);
//   5. a second scan gives each row its first vertex in the block and the block its totals (rows, vertices, polygon vertices).
// The count kernel stores the totals per block; after a scan over blocks (costmap_obstacles_scan_kernel) the write kernel runs the same
// cmp_block again and writes each row's first-vertex offset and its vertices' world coordinates into scratch. The two kernels call the
// same function, so the counts and the writes cannot disagree. The forms for a scene set (at the end of this file) run the same
// cmp_block and the same write pass behind a per-scene record.
#pragma once
#include "teb_costmap_obstacles.hpp"

namespace tebamd {

// CmpGeom, CmpSceneRec and the kCmp* constants: teb_costmap_pods.hpp; the rules that fill them: teb_costmap_host.hpp (polygon_blocks, PolygonRows::layout)

// The converted rows in scratch: off[row] = its first vertex, x / y the vertices (world coordinates) of all rows in row order.
struct CmpOut {
  int* off;
  double *x, *y;
};

struct CmpLds {
  int lab[kCmpSlots];    // kept cell: the slot of its component's root; -1: no kept cell
  int seg[kCmpSlots];    // root: its last column, then the exclusive scan (rank << 16 | first candidate entry)
  int chain[kCmpSlots];  // root: columns | lower chain length << 8 | upper chain length << 16
  int vtx[kCmpSlots];    // root: exclusive scan (vertices << 16 | polygon vertices)
  int lo[kCmpSlots];     // candidate entries (packed dx << 6 | ddy): the lowest cell of a column, then the lower chain
  int hi[kCmpSlots];     // the highest cell of a column, then the upper chain (stacked from the segment's end down)
  int part[kCmpThreads];
};

__device__ __forceinline__ int cmp_ld(const int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// Root of x. Parents only ever decrease (every write is an atomicMin towards an ancestor), so the walk ends, and the root a component
// ends with is its smallest slot.
__device__ __forceinline__ int cmp_find(int* lab, int x) {
  int p = cmp_ld(&lab[x]);
  while (p != x) {
    const int gp = cmp_ld(&lab[p]);
    if (gp != p) atomicMin(&lab[x], gp);   // path splitting: x skips to its grandparent
    x = p;
    p = gp;
  }
  return x;
}

// Merges the components of a and b: the larger root goes under the smaller one; a failed link (the root moved meanwhile) retries from
// where it was linked to.
__device__ __forceinline__ void cmp_unite(int* lab, int a, int b) {
  while (true) {
    a = cmp_find(lab, a);
    b = cmp_find(lab, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&lab[b], a);
    if (old == b) return;
    b = old;
  }
}

// Exclusive scan of v[0 .. kCmpSlots) in place (each lane one contiguous run of kCmpPer slots); returns the total to every lane.
__device__ __forceinline__ int cmp_block_scan(int* v, int* part) {
  const int tid = threadIdx.x, b = tid * kCmpPer;
  int s = 0;
  for (int i = 0; i < kCmpPer; ++i) s += v[b + i];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < kCmpThreads; d <<= 1) {   // inclusive Hillis-Steele scan of the run sums
    const int u = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += u;
    __syncthreads();
  }
  int run = tid > 0 ? part[tid - 1] : 0;
  for (int i = 0; i < kCmpPer; ++i) {
    const int c = v[b + i];
    v[b + i] = run;
    run += c;
  }
  const int total = part[kCmpThreads - 1];
  __syncthreads();
  return total;
}

__device__ __forceinline__ int cmp_cross(int o, int a, int b) {   // (a - o) x (b - o) of packed (dx << 6 | ddy) points: exact
  const int ox = o >> 6, oy = o & 63;
  return ((a >> 6) - ox) * ((b & 63) - oy) - ((a & 63) - oy) * ((b >> 6) - ox);
}

// The rows of block blk in LDS (steps 1 - 5 above). Returns (rows, vertices, polygon vertices) of the block.
__device__ void cmp_block(const GridDev& g, const CmoFilter& f, const CmpGeom& q, int blk, CmpLds& s, int& rows, int& verts,
                          int& pverts) {
  const int T = q.T, TT = T * T;
  const int tx = blk / q.nby, ty0 = (blk % q.nby) * q.k;
  const int x0 = tx * T, w = min(T, q.ncols - x0), kb = min(q.k, q.nty - ty0), y0 = ty0 * T;
  const int tid = threadIdx.x;
  // 1. kept mask
  for (int i = tid; i < kCmpSlots; i += kCmpThreads) {
    const int j = i / TT, dx = (i - j * TT) / T, my = y0 + j * T + (i - j * TT - dx * T);
    double wx, wy;
    const bool kept = j < kb && dx < w && my < q.nrows && costmap_point_obstacle(g, f, x0 + dx, my, wx, wy);
    s.lab[i] = kept ? i : -1;
    s.seg[i] = -1;
    s.lo[i] = 0x7fffffff;
    s.hi[i] = -1;
  }
  __syncthreads();
  // 2. components of each tile
  for (int i = tid; i < kCmpSlots; i += kCmpThreads) {
    if (cmp_ld(&s.lab[i]) < 0) continue;
    const int dx = (i % TT) / T, ddy = i % T;
    if (ddy + 1 < T && cmp_ld(&s.lab[i + 1]) >= 0) cmp_unite(s.lab, i, i + 1);
    if (dx + 1 < T) {
      for (int e = -1; e <= 1; ++e) {
        if (ddy + e < 0 || ddy + e >= T) continue;
        const int n = i + T + e;
        if (cmp_ld(&s.lab[n]) >= 0) cmp_unite(s.lab, i, n);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < kCmpSlots; i += kCmpThreads)
    if (cmp_ld(&s.lab[i]) >= 0) __atomic_store_n(&s.lab[i], cmp_find(s.lab, i), __ATOMIC_RELAXED);
  __syncthreads();
  // 3. last column of each component, then rank and candidate segment
  for (int i = tid; i < kCmpSlots; i += kCmpThreads)
    if (s.lab[i] >= 0) atomicMax(&s.seg[s.lab[i]], (i % TT) / T);
  __syncthreads();
  for (int i = tid; i < kCmpSlots; i += kCmpThreads) {
    const int cols = s.lab[i] == i ? s.seg[i] - (i % TT) / T + 1 : 0;
    s.chain[i] = cols;
    s.seg[i] = cols > 0 ? (1 << 16) + cols : 0;
  }
  __syncthreads();
  rows = cmp_block_scan(s.seg, s.part) >> 16;
  for (int i = tid; i < kCmpSlots; i += kCmpThreads) {
    const int r = s.lab[i];
    if (r < 0) continue;
    const int dx = (i % TT) / T, e = (s.seg[r] & 0xffff) + dx - (r % TT) / T, p = (dx << 6) | (i % T);
    atomicMin(&s.lo[e], p);
    atomicMax(&s.hi[e], p);
  }
  __syncthreads();
  // 4. hulls: one lane per component
  for (int i = tid; i < kCmpSlots; i += kCmpThreads) {
    s.vtx[i] = 0;
    if (s.lab[i] != i) continue;
    const int c = s.chain[i], base = s.seg[i] & 0xffff;
    int* L = s.lo + base;
    int kl = 0;
    for (int t = 0; t < c; ++t) {
      const int p = L[t];
      while (kl >= 2 && cmp_cross(L[kl - 2], L[kl - 1], p) <= 0) --kl;
      L[kl++] = p;
    }
    int* U = s.hi + base + c - 1;   // U[-m]: the m-th entry of the upper chain
    int ku = 0;
    for (int t = c - 1; t >= 0; --t) {
      const int p = s.hi[base + t];
      while (ku >= 2 && cmp_cross(U[-(ku - 2)], U[-(ku - 1)], p) <= 0) --ku;
      U[-ku] = p;
      ++ku;
    }
    const int nl = kl - (L[kl - 1] == U[0] ? 1 : 0), nu = ku - (U[-(ku - 1)] == L[0] ? 1 : 0);
    const int nv = nl + nu > 0 ? nl + nu : 1;   // one cell: one vertex
    s.chain[i] = c | (kl << 8) | (ku << 16);
    s.vtx[i] = (nv << 16) | (nv >= 3 ? nv : 0);
  }
  __syncthreads();
  // 5. vertex offsets and totals
  const int tv = cmp_block_scan(s.vtx, s.part);
  verts = tv >> 16;
  pverts = tv & 0xffff;
}

__global__ void __launch_bounds__(kCmpThreads) costmap_polygons_count_kernel(GridDev g, CmoFilter f, CmpGeom q, int nblk, int* cnt) {
  __shared__ CmpLds s;
  int rows, verts, pverts;
  cmp_block(g, f, q, blockIdx.x, s, rows, verts, pverts);
  if (threadIdx.x == 0) {   // three arrays of nblk + 1 (the scan appends each total)
    cnt[blockIdx.x] = rows;
    cnt[(nblk + 1) + blockIdx.x] = verts;
    cnt[2 * (nblk + 1) + blockIdx.x] = pverts;
  }
}

// The write pass of a block after cmp_block: every row's first-vertex offset and its vertices' world coordinates. off_rows / off_verts:
// the block's first row and first vertex (the scanned counts); o: where row 0 and vertex 0 of the table go.
__device__ __forceinline__ void cmp_write_block(const GridDev& g, const CmpGeom& q, int blk, const CmpLds& s, const int* off_rows,
                                                const int* off_verts, const CmpOut& o) {
  const int T = q.T, TT = T * T;
  const int x0 = (blk / q.nby) * T, y0 = (blk % q.nby) * q.k * T;
  const int row0 = off_rows[blk], v0 = off_verts[blk];
  for (int i = threadIdx.x; i < kCmpSlots; i += kCmpThreads) {
    if (s.lab[i] != i) continue;
    const int c = s.chain[i] & 0xff, kl = (s.chain[i] >> 8) & 0xff, ku = s.chain[i] >> 16, base = s.seg[i] & 0xffff;
    const int* L = s.lo + base;
    const int* U = s.hi + base + c - 1;
    const int nl = kl - (L[kl - 1] == U[0] ? 1 : 0), nu = ku - (U[-(ku - 1)] == L[0] ? 1 : 0);
    const int ym = y0 + (i / TT) * T;   // first row of the component's tile
    int v = v0 + (s.vtx[i] >> 16);
    o.off[row0 + (s.seg[i] >> 16)] = v;
    auto put = [&](int p) { costmap_cell_centre(g, x0 + (p >> 6), ym + (p & 63), o.x[v], o.y[v]); ++v; };
    if (nl + nu == 0) put(L[0]);
    for (int t = 0; t < nl; ++t) put(L[t]);
    for (int t = 0; t < nu; ++t) put(U[-t]);
  }
}

__global__ void __launch_bounds__(kCmpThreads) costmap_polygons_write_kernel(GridDev g, CmoFilter f, CmpGeom q, int nblk, const int* off,
                                                                             CmpOut o) {
  __shared__ CmpLds s;
  int rows, verts, pverts;
  cmp_block(g, f, q, blockIdx.x, s, rows, verts, pverts);
  cmp_write_block(g, q, blockIdx.x, s, off, off + (nblk + 1), o);
}

// ---- the scene set (teb_amd_set_scenes_from_costmap_polygons): the passes over the grids of a costmap set (teb_amd_set_costmaps), one
// launch each. The launch is flat: the blocks of the scenes one after the other, as many workgroups as the set has blocks (a workgroup
// holds 97 KB of LDS and so runs alone on its CU: none is started for nothing). A workgroup finds its scene by a search over the prefix
// array of block counts that depends on blockIdx.x alone, so the scene's record is uniform over the workgroup and arrives through scalar
// loads. The blocks are the single-scene blocks: a scene's counts, offsets and vertices are those of a handle that holds only its grid.
// The scene of flat block b: the last s with blk0[s] <= b (blk0: n + 1 entries, blk0[n] = blocks of the set > b), which skips the scenes
// without blocks.
__device__ __forceinline__ int cmp_scene_of_block(const int* __restrict__ blk0, int n, int b) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk0[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}

// cnt: three arrays (rows, vertices, polygon vertices) of ncnt = sum of (nblk + 1) counters each
__global__ void __launch_bounds__(kCmpThreads) costmap_polygons_count_fleet_kernel(const CmpSceneRec* __restrict__ recs,
                                                                                   const int* __restrict__ blk0, int n_scenes, int ncnt,
                                                                                   int* cnt) {
  __shared__ CmpLds s;
  const CmpSceneRec r = recs[cmp_scene_of_block(blk0, n_scenes, blockIdx.x)];   // by value: the record lives in scalar registers
  const int blk = blockIdx.x - r.blk0;
  int rows, verts, pverts;
  cmp_block(r.g, r.f, r.q, blk, s, rows, verts, pverts);
  if (threadIdx.x == 0) {
    int* c = cnt + r.cnt0 + blk;
    c[0] = rows;
    c[ncnt] = verts;
    c[2 * (size_t)ncnt] = pverts;
  }
}
// one workgroup per (scene, array): blockIdx.x = 3 * scene + array. The total lands behind the scene's counters and in
// totals[array * n_scenes + scene] - what the host reads, in one copy.
__global__ void __launch_bounds__(kCmoScanThreads) costmap_polygons_scan_fleet_kernel(const CmpSceneRec* __restrict__ recs, int n_scenes,
                                                                                      int ncnt, int* cnt, int* totals) {
  __shared__ int part[kCmoScanThreads];
  const int sc = blockIdx.x / 3, a = blockIdx.x % 3;
  const CmpSceneRec& r = recs[sc];
  costmap_obstacles_scan_group(cnt + (size_t)a * ncnt + r.cnt0, r.nblk, part);
  if (threadIdx.x == kCmoScanThreads - 1) totals[a * n_scenes + sc] = part[threadIdx.x];
}
// o: the scratch of the whole set; a row's first-vertex offset counts from the scene's first vertex
__global__ void __launch_bounds__(kCmpThreads) costmap_polygons_write_fleet_kernel(const CmpSceneRec* __restrict__ recs,
                                                                                   const int* __restrict__ blk0, int n_scenes, int ncnt,
                                                                                   const int* cnt, CmpOut o) {
  __shared__ CmpLds s;
  const CmpSceneRec r = recs[cmp_scene_of_block(blk0, n_scenes, blockIdx.x)];   // by value: the record lives in scalar registers
  const int blk = blockIdx.x - r.blk0;
  int rows, verts, pverts;
  cmp_block(r.g, r.f, r.q, blk, s, rows, verts, pverts);
  cmp_write_block(r.g, r.q, blk, s, cnt + r.cnt0, cnt + ncnt + r.cnt0, CmpOut{o.off + r.row0, o.x + r.vtx0, o.y + r.vtx0});
}

}  // namespace tebamd
