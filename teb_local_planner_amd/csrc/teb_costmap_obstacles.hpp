// teb_costmap_obstacles.hpp — TebLocalPlannerROS::updateObstacleContainerWithCostmap (src/teb_local_planner_ros.cpp:478-504) on the
// costmap grid of teb_amd_set_costmap: one PointObstacle per LETHAL_OBSTACLE cell that is not far behind the robot, written straight
// into the rows of the handle's obstacle table, in the reference's order.
//
// The reference loops mx (outer) over the columns and my (inner) over the rows of a row-major grid, so the table order is transposed
// with respect to memory. This is an order-preserving stream compaction in three launches:
//   count: one lane per (column, chunk of rows); lanes run along mx, so a wave reads 64 neighbouring bytes of one row at a time.
//          Each lane writes the number of kept cells of its chunk to cnt[mx * nchunks + chunk] - (column, chunk) order is table order.
//   scan:  one workgroup turns cnt into exclusive offsets in place and appends the total (cnt[ncols * nchunks]), the only value the
//          host reads back before it decides whether the table fits.
//   write: each lane walks its chunk again and writes its kept cells from its offset on, in row order.
// Both passes evaluate the one predicate below, so the counts and the writes cannot disagree. Every kernel is a thin wrapper round a
// __forceinline__ body; the forms for a scene set (at the end of this file) run the same bodies behind a per-scene record.
#pragma once
#include "teb_feasibility.hpp"
#include "teb_costmap_pods.hpp"

namespace tebamd {

// GridDev, CmoFilter, CmoRows, CmoSceneRec and kCmoThreads / kCmoScanThreads: teb_costmap_pods.hpp; the rules that fill them: teb_costmap_host.hpp

// costmap_2d::Costmap2D::mapToWorld: the centre of cell (mx, my) (also the vertices of teb_costmap_polygons.hpp)
__device__ __forceinline__ void costmap_cell_centre(const GridDev& g, int mx, int my, double& wx, double& wy) {
  wx = g.ox + (mx + 0.5) * g.res;
  wy = g.oy + (my + 0.5) * g.res;
}

// Cell (mx, my) becomes a point obstacle at (wx, wy). Plain IEEE products and sums (-ffp-contract=off): Eigen's dot and norm of a
// Vector2d; sqrt is correctly rounded.
__device__ __forceinline__ bool costmap_point_obstacle(const GridDev& g, const CmoFilter& f, int mx, int my, double& wx, double& wy) {
  if (g.cells[(size_t)my * (size_t)g.sx + (size_t)mx] != 254) return false;   // costmap_2d::LETHAL_OBSTACLE
  costmap_cell_centre(g, mx, my, wx, wy);
  const double dx = wx - f.rx, dy = wy - f.ry;
  return !(dx * f.c + dy * f.s < 0 && sqrt(dx * dx + dy * dy) > f.dist);
}

// One lane of the count pass: lane t of the scene's ncols * nchunks lanes (lanes beyond them do nothing).
__device__ __forceinline__ void costmap_obstacles_count_lane(const GridDev& g, const CmoFilter& f, int ncols, int nrows, int chunk, int nchunks,
                                                             int* cnt, size_t t) {
  if (t >= (size_t)ncols * nchunks) return;
  const int mx = (int)(t % ncols), ch = (int)(t / ncols);
  const int y1 = min(ch * chunk + chunk, nrows);
  int k = 0;
  double wx, wy;
  for (int my = ch * chunk; my < y1; ++my) k += costmap_point_obstacle(g, f, mx, my, wx, wy) ? 1 : 0;
  cnt[(size_t)mx * nchunks + ch] = k;
}
__global__ void __launch_bounds__(kCmoThreads) costmap_obstacles_count_kernel(GridDev g, CmoFilter f, int ncols, int nrows, int chunk,
                                                                              int nchunks, int* cnt) {
  costmap_obstacles_count_lane(g, f, ncols, nrows, chunk, nchunks, cnt, (size_t)blockIdx.x * kCmoThreads + threadIdx.x);
}

// Exclusive scan of cnt[0 .. n) in place, total to cnt[n]: every thread sums one contiguous segment, the workgroup scans the segment
// sums in LDS, every thread rewrites its segment. n is at most 64 K values up to a 2048 x 2048 grid, 262 K at 4096 x 4096.
__device__ __forceinline__ void costmap_obstacles_scan_group(int* cnt, int n, int* part /* LDS [kCmoScanThreads] */) {
  const int tid = threadIdx.x;
  const int per = (n + kCmoScanThreads - 1) / kCmoScanThreads;
  const int b = min(tid * per, n), e = min(b + per, n);
  int s = 0;
  for (int i = b; i < e; ++i) s += cnt[i];
  part[tid] = s;
  __syncthreads();
  for (int d = 1; d < kCmoScanThreads; d <<= 1) {   // inclusive Hillis-Steele scan of the segment sums
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = tid > 0 ? part[tid - 1] : 0;
  for (int i = b; i < e; ++i) {
    const int c = cnt[i];
    cnt[i] = run;
    run += c;
  }
  if (tid == kCmoScanThreads - 1) cnt[n] = part[tid];
}
__global__ void __launch_bounds__(kCmoScanThreads) costmap_obstacles_scan_kernel(int* cnt, int n) {
  __shared__ int part[kCmoScanThreads];
  costmap_obstacles_scan_group(cnt, n, part);
}

// One lane of the write pass: its kept cells go to sink(o, wx, wy) from its offset on, in row order.
template <class Sink>
__device__ __forceinline__ void costmap_obstacles_write_lane(const GridDev& g, const CmoFilter& f, int ncols, int nrows, int chunk, int nchunks,
                                                             const int* off, size_t t, Sink&& sink) {
  if (t >= (size_t)ncols * nchunks) return;
  const int mx = (int)(t % ncols), ch = (int)(t / ncols);
  const int y1 = min(ch * chunk + chunk, nrows);
  int o = off[(size_t)mx * nchunks + ch];
  double wx, wy;
  for (int my = ch * chunk; my < y1; ++my) {
    if (!costmap_point_obstacle(g, f, mx, my, wx, wy)) continue;
    sink(o, wx, wy);
    ++o;
  }
}
__global__ void __launch_bounds__(kCmoThreads) costmap_obstacles_write_kernel(GridDev g, CmoFilter f, int ncols, int nrows, int chunk,
                                                                              int nchunks, const int* off, CmoRows r) {
  costmap_obstacles_write_lane(g, f, ncols, nrows, chunk, nchunks, off, (size_t)blockIdx.x * kCmoThreads + threadIdx.x,
                               [&r](int o, double wx, double wy) {
    // what teb_amd_set_obstacles derives for a TEB_AMD_OBST_POINT row with radius 0, velocity 0, not dynamic, no vertices
    r.type[o] = TEB_AMD_OBST_POINT; r.dyn[o] = 0; r.voff[o] = 0;
    r.ax[o] = wx; r.ay[o] = wy; r.bx[o] = 0.0; r.by[o] = 0.0; r.rad[o] = 0.0; r.vx[o] = 0.0; r.vy[o] = 0.0;
    r.cx[o] = wx; r.cy[o] = wy; r.brad[o] = 0.0;
  });
}

// ---- the scene set (teb_amd_set_scenes_from_costmaps): the three passes over the grids of a costmap set (teb_amd_set_costmaps), one
// launch each. Every scene has a record; blockIdx.y (count, write) or blockIdx.x (scan) selects it, so the record is uniform over the
// workgroup and arrives through scalar loads. The lanes are the single-scene lanes: a scene's counts, offsets and points are those of
// a handle that holds only its grid.
// (CmoSceneRec: the lanes are point_lanes of teb_costmap_host.hpp on the scene's grid, laid out by PointRows::layout.)
// grid = (blocks over the scene with the most lanes, scenes): a workgroup beyond its scene's lanes returns at once
__global__ void __launch_bounds__(kCmoThreads) costmap_obstacles_count_fleet_kernel(const CmoSceneRec* __restrict__ recs, int* cnt) {
  const CmoSceneRec& q = recs[blockIdx.y];
  if ((size_t)blockIdx.x * kCmoThreads >= (size_t)q.ncols * q.nchunks) return;
  costmap_obstacles_count_lane(q.g, q.f, q.ncols, q.nrows, q.chunk, q.nchunks, cnt + q.cnt_off, (size_t)blockIdx.x * kCmoThreads + threadIdx.x);
}
// one workgroup per scene; the scene's total lands behind its counters and in totals[scene]
__global__ void __launch_bounds__(kCmoScanThreads) costmap_obstacles_scan_fleet_kernel(const CmoSceneRec* __restrict__ recs, int* cnt, int* totals) {
  __shared__ int part[kCmoScanThreads];
  const CmoSceneRec& q = recs[blockIdx.x];
  costmap_obstacles_scan_group(cnt + q.cnt_off, q.ncols * q.nchunks, part);
  if (threadIdx.x == kCmoScanThreads - 1) totals[blockIdx.x] = part[threadIdx.x];   // what the host reads: one int per scene, one copy
}
__global__ void __launch_bounds__(kCmoThreads) costmap_obstacles_write_fleet_kernel(const CmoSceneRec* __restrict__ recs, const int* cnt,
                                                                                    double* __restrict__ px, double* __restrict__ py) {
  const CmoSceneRec& q = recs[blockIdx.y];
  if ((size_t)blockIdx.x * kCmoThreads >= (size_t)q.ncols * q.nchunks) return;
  double* ox = px + q.out_off;
  double* oy = py + q.out_off;
  costmap_obstacles_write_lane(q.g, q.f, q.ncols, q.nrows, q.chunk, q.nchunks, cnt + q.cnt_off, (size_t)blockIdx.x * kCmoThreads + threadIdx.x,
                               [ox, oy](int o, double wx, double wy) { ox[o] = wx; oy[o] = wy; });
}

}  // namespace tebamd
