// teb_costmap_pods.hpp — what the kernels of the costmap conversion (teb_costmap_obstacles.hpp, teb_costmap_polygons.hpp) and of the
// feasibility check (teb_feasibility.hpp) read: kernel arguments and per-scene records, filled by the host rules of
// teb_costmap_host.hpp. Plain structs and constants, nothing else: any compiler may include it.
#pragma once

namespace tebamd {

// ---- what the kernels read: layouts are part of the launch contract ------------------------------------------------------------------
// a costmap_2d grid: row-major cells (device memory), size, resolution and origin
struct GridDev {
  const unsigned char* cells;
  int sx, sy;
  double res, ox, oy;
};
static_assert(sizeof(GridDev) == 40, "GridDev is a kernel argument");

// robot_pose_ and costmap_obstacles_behind_robot_dist; (c, s) = PoseSE2::orientationUnitVec (pose_se2.h:215), computed on the host
// with std::cos / std::sin so that the bits are glibc's (costmap_filter)
struct CmoFilter {
  double rx, ry, c, s, dist;
};
static_assert(sizeof(CmoFilter) == 40, "CmoFilter is a kernel argument");

// The rows of the obstacle table the single-scene write pass of the point route fills (SceneDev order of teb_amd_set_obstacles).
struct CmoRows {
  int *type, *dyn, *voff;
  double *ax, *ay, *bx, *by, *rad, *vx, *vy, *cx, *cy, *brad;
};
static_assert(sizeof(CmoRows) == 13 * sizeof(void*), "CmoRows is a kernel argument");

constexpr int kCmoThreads = 256;
constexpr int kCmoScanThreads = 1024;
constexpr int kCmpThreads = 256;
constexpr int kCmpSlots = 4096;                       // cells of a block: one 64 x 64 tile at most
constexpr int kCmpPer = kCmpSlots / kCmpThreads;      // slots per lane in the block scans
constexpr int kCmpMaxTile = 64;

// The block geometry of the polygon route: tiles of T cells, k tiles per block, ntx x nby blocks over the visit domain ncols x nrows.
struct CmpGeom {
  int ncols, nrows, T, k, nty, nby;
};
static_assert(sizeof(CmpGeom) == 24, "CmpGeom is a kernel argument");

// A scene of a set on the point route (the single scene is a set of one whose record travels by value).
struct CmoSceneRec {
  GridDev g;
  CmoFilter f;
  int ncols, nrows, chunk, nchunks;   // point_lanes on this grid (0 lanes: a grid without interior columns / rows)
  int cnt_off;                        // first of the scene's ncols * nchunks + 1 counters
  int out_off;                        // first point of the scene in the scratch of the write pass (prefix of the totals)
};
static_assert(sizeof(CmoSceneRec) == 104, "CmoSceneRec is read by the fleet kernels of teb_costmap_obstacles.hpp");

// A scene of a set on the polygon route.
struct CmpSceneRec {
  GridDev g;
  CmoFilter f;
  CmpGeom q;      // the scene's own tile size: T, k = kCmpSlots / T^2
  int blk0;       // the scene's first block in the flat block list of the set
  int nblk;       // its blocks (0: a grid without a visit domain)
  int cnt0;       // first of the scene's nblk + 1 counters in each of the three count arrays
  int row0, vtx0; // write pass: the scene's first row / first vertex in the scratch of the whole set
};
static_assert(sizeof(CmpSceneRec) == 128, "CmpSceneRec is read by the fleet kernels of teb_costmap_polygons.hpp");

}  // namespace tebamd
