// teb_plan_window.hpp — device library: every robot's local plan window from its resident global plan, one workgroup per robot.
//
// What TebLocalPlannerROS::computeVelocityCommands runs before planner_->plan() (src/teb_local_planner_ros.cpp:268-340), for a fleet:
//   pruneGlobalPlan :669-690, transformGlobalPlan :729-797, updateViaPointsContainer :627-645, estimateLocalGoalOrientation :827-871,
//   the start replacement :336-340 and the transformed global goal of the goal-reached test :291-292.
// The reference runs every step as a sequential scan; here every DECISION (an index, a count, a cut) is the sequential one bit for bit:
//   - first matches (prune, distance cut) are ballots over 256-pose chunks with a workgroup-uniform early exit;
//   - the closest pose with its early break is a prefix-minimum scan (comparisons only: exactly the sequential minimum), wave shuffles
//     inside a wave, LDS across the four waves, the running minimum and the reached flag carried from chunk to chunk;
//   - plan_length is a floating-point sum whose value decides an index: ONE lane adds the segment lengths, which the others computed
//     in parallel, in the reference's order - no tree, no scan;
//   - the via-point chain is serial across accepted points; one wave tests 64 candidates per step and takes the first ballot bit.
// fp64, one IEEE operation per source operation of the restatement (tests/plan_window_cases.py); the library is built with
// -ffp-contract=off and the kernel body repeats it (a pragma of that body alone: nothing an including unit defines later is touched),
// so no product is fused into a sum there. The helpers above the kernel compare and shuffle; they have no arithmetic to fuse.
#pragma once
#include "teb_edges.hpp"

namespace tebamd {

constexpr int kPwThreads = 256;
constexpr int kPwWaves = kPwThreads / 64;

// what teb_amd_plan_windows downloads per robot (one record, 80 bytes)
struct PlanWinOut {
  int window_count;   // poses of the delivered window (after the start insertion); 0: empty plan
  int goal_idx;       // index of the local goal in the pruned plan
  int cursor;         // the new begin
  int pruned;         // pruneGlobalPlan's return value
  int via_count;
  int alloc;          // A: the robot's block in the pack buffer is [win_x (A) | win_y (A) | win_yaw (A) | via_x (A) | via_y (A)]
  long long off;      // first double of that block, -1: none
  double goal[3];
  double global_goal[3];
};

struct PlanWinArgs {
  const double* px; const double* py; const double* pyaw;   // the plans one after the other
  const long long* first;   // [n] first pose of plan r
  const int* count;         // [n] poses of plan r
  int* cursor;              // [n] in / out
  const double* pose;       // [3 n] robot pose, global frame
  const double* tf;         // [5 n] (cos, sin, tx, ty, yaw_tf) or nullptr = identity
  const double* thr;        // [n] dist_threshold
  double prune_distance, max_plan_length, via_sep;
  int overwrite_orientation, moving_average_length;
  PlanWinOut* out;          // [n]
  double* pack;             // the windows and via-points of the call, one block per robot at the offset its ticket gave it
  unsigned long long* ticket;   // doubles handed out so far (zeroed before the launch)
  long long pack_capacity;
};

__device__ __forceinline__ int pw_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// inclusive prefix minimum over the 64 lanes of a wave (strict '<': ties keep the earlier value, which is the same value)
__device__ __forceinline__ double pw_wave_prefix_min(double v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double u = __shfl_up(v, o);
    if (lane >= o && u < v) v = u;
  }
  return v;
}
// position of the first set bit of the four wave ballots, kPwThreads if none
__device__ __forceinline__ int pw_first_bit(const unsigned long long* m) {
  for (int w = 0; w < kPwWaves; ++w)
    if (m[w]) return w * 64 + __ffsll((long long)m[w]) - 1;
  return kPwThreads;
}
// position of the last set bit below `end`, -1 if none
__device__ __forceinline__ int pw_last_bit_below(const unsigned long long* m, int end) {
  for (int w = kPwWaves - 1; w >= 0; --w) {
    const int lo = w * 64;
    if (end <= lo) continue;
    unsigned long long v = m[w];
    if (end < lo + 64) v &= (1ull << (end - lo)) - 1ull;
    if (v) return lo + 63 - __clzll((long long)v);
  }
  return -1;
}

__global__ void __launch_bounds__(kPwThreads) plan_window_kernel(const PlanWinArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_d[kPwThreads];                  // squared distances / segment lengths of the chunk
  __shared__ double s_wmin[kPwWaves];
  __shared__ unsigned long long s_m0[kPwWaves], s_m1[kPwWaves], s_m2[kPwWaves];
  __shared__ double s_carry[2];                       // plan_length, and the value of the closest pose
  __shared__ int s_int[4];
  __shared__ long long s_off;

  const int r = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = pw_uniform(tid >> 6);
  const int n_tot = a.count[r];
  int begin = a.cursor[r];
  const double* X = a.px + a.first[r];
  const double* Y = a.py + a.first[r];
  const double* YAW = a.pyaw + a.first[r];
  PlanWinOut* out = a.out + r;

  if (n_tot - begin <= 0) {   // global_plan.empty(): prune returns true (:659), transformGlobalPlan sets goal_idx = 0 and fails (:713-718)
    if (tid == 0) {
      out->window_count = 0; out->goal_idx = 0; out->cursor = begin; out->pruned = 1; out->via_count = 0; out->alloc = 0; out->off = -1;
      for (int k = 0; k < 3; ++k) { out->goal[k] = 0.0; out->global_goal[k] = 0.0; }
    }
    return;
  }

  // ---- 1. the robot in the plan frame: R^T (g - t) ---------------------------------------------------------------------------------
  const double gx = a.pose[3 * r], gy = a.pose[3 * r + 1], gth = a.pose[3 * r + 2];
  const double tc = a.tf ? a.tf[5 * r] : 1.0, ts = a.tf ? a.tf[5 * r + 1] : 0.0, tx = a.tf ? a.tf[5 * r + 2] : 0.0,
               ty = a.tf ? a.tf[5 * r + 3] : 0.0, tyaw = a.tf ? a.tf[5 * r + 4] : 0.0;
  const double ddx = gx - tx, ddy = gy - ty;
  const double rx = tc * ddx + ts * ddy;
  const double ry = tc * ddy - ts * ddx;

  // ---- 2. prune: the first j >= begin with dx^2 + dy^2 < prune_distance^2 ------------------------------------------------------------
  int pruned = 0;
  {
    const double thr_sq = a.prune_distance * a.prune_distance;
    for (int base = begin; base < n_tot; base += kPwThreads) {
      const int j = base + tid;
      bool hit = false;
      if (j < n_tot) {
        const double dx = rx - X[j], dy = ry - Y[j];
        hit = dx * dx + dy * dy < thr_sq;
      }
      const unsigned long long m = __ballot(hit);
      if (lane == 0) s_m0[wv] = m;
      __syncthreads();
      const int f = pw_uniform(pw_first_bit(s_m0));
      __syncthreads();
      if (f < kPwThreads) { begin = base + f; pruned = 1; break; }
    }
  }
  X += begin; Y += begin; YAW += begin;
  const int N = n_tot - begin;   // the pruned plan: every index below is relative to the cursor

  // ---- 3. the closest pose, with the early break ------------------------------------------------------------------------------------
  int ci = 0;
  double sq_dist = 1e10;
  {
    bool reached = false;
    for (int base = 0; base < N; base += kPwThreads) {
      const int j = base + tid;
      const bool valid = j < N;
      double d = 1.7976931348623157e308;
      if (valid) {
        const double dx = rx - X[j], dy = ry - Y[j];
        d = dx * dx + dy * dy;
      }
      s_d[tid] = d;
      const double inc = pw_wave_prefix_min(d, lane);
      if (lane == 63) s_wmin[wv] = inc;
      double before = __shfl_up(inc, 1);   // minimum of the lanes before this one (lane 0: none)
      __syncthreads();
      double head = sq_dist;               // the running minimum up to the first lane of this wave
      for (int w = 0; w < wv; ++w) { const double u = s_wmin[w]; if (u < head) head = u; }
      const double m_prev = (lane == 0 || !(before < head)) ? head : before;
      const bool is_new = valid && d < m_prev;
      const bool reach = is_new && d < 0.05;
      const unsigned long long m_new = __ballot(is_new), m_reach = __ballot(reach);
      if (lane == 0) { s_m0[wv] = m_new; s_m1[wv] = m_reach; }
      __syncthreads();
      bool reached_before = reached;
      for (int w = 0; w < wv; ++w) reached_before = reached_before || s_m1[w] != 0;
      reached_before = reached_before || (s_m1[wv] & ((1ull << lane) - 1ull)) != 0;
      const bool brk = valid && reached_before && d > m_prev;
      const unsigned long long m_brk = __ballot(brk);
      if (lane == 0) s_m2[wv] = m_brk;
      __syncthreads();
      const int jb = pw_uniform(pw_first_bit(s_m2));            // kPwThreads: the scan goes on
      const int last_new = pw_uniform(pw_last_bit_below(s_m0, jb));
      if (last_new >= 0) { ci = base + last_new; sq_dist = s_d[last_new]; }
      reached = reached || pw_first_bit(s_m1) < kPwThreads;
      __syncthreads();
      if (jb < kPwThreads) break;
    }
  }

  // ---- 4. the window [ci, k_end): the distance cut is a first match, plan_length one lane's sum in the reference's order ---------------
  int k_end = ci;
  {
    const double thr = a.thr[r];
    const double thr_sq = thr * thr;
    const double max_len = a.max_plan_length;
    if (sq_dist <= thr_sq) {
      if (tid == 0) s_carry[0] = 0.0;
      for (int base = ci; base < N; base += kPwThreads) {
        const int k = base + tid;
        bool cut = false;
        double seg = 0.0;
        if (k < N) {
          const double xk = X[k], yk = Y[k];
          const double dx = rx - xk, dy = ry - yk;
          cut = !(dx * dx + dy * dy <= thr_sq);   // pose k is pushed, the loop stops after it
          if (k > 0 && max_len > 0) {
            const double ex = xk - X[k - 1], ey = yk - Y[k - 1];
            seg = sqrt(ex * ex + ey * ey);        // distance_points2d(plan[k - 1], plan[k])
          }
        }
        s_d[tid] = seg;
        const unsigned long long m = __ballot(cut);
        if (lane == 0) s_m0[wv] = m;
        __syncthreads();
        const int fc = pw_uniform(pw_first_bit(s_m0));
        int last = N - base < kPwThreads ? N - base : kPwThreads;   // poses of this chunk that can be pushed
        bool stop = last < kPwThreads || N - base == kPwThreads;
        if (fc < last) { last = fc + 1; stop = true; }
        if (max_len > 0) {
          if (tid == 0) {
            double pl = s_carry[0];
            int q = 0;
            for (; q < last; ++q) {
              if (!(pl <= max_len)) break;
              pl += s_d[q];                       // (k = 0 carries a zero: no segment before the first pose)
            }
            s_carry[0] = pl;
            s_int[0] = q;
          }
          __syncthreads();
          const int q = pw_uniform(s_int[0]);
          if (q < last) { last = q; stop = true; }
        }
        k_end = base + last;
        __syncthreads();
        if (stop) break;
      }
    }
  }
  int W = k_end - ci;
  int goal_idx = k_end - 1, src0 = ci;
  if (W == 0) { W = 1; goal_idx = N - 1; src0 = N - 1; }   // empty window: the global goal is injected (:784-792)
  const int shift = W == 1 ? 1 : 0;                         // a one-pose window gets the start inserted in front (:336-339)
  const int A = W + 1;

  // the robot's block of the pack buffer
  if (tid == 0) {
    const long long off = (long long)atomicAdd(a.ticket, 5ull * (unsigned long long)A);
    s_off = off + 5ll * A <= a.pack_capacity ? off : -1;
  }
  __syncthreads();
  const long long off = s_off;
  const bool fits = off >= 0;
  double* wx = a.pack + (fits ? off : 0);
  double* wy = wx + A;
  double* wyaw = wy + A;
  double* vx = wyaw + A;
  double* vy = vx + A;

  // ---- 5. transform: R p + t, yaw + yaw_tf -------------------------------------------------------------------------------------------
  if (fits) {
    for (int q = tid; q < W; q += kPwThreads) {
      const double x = X[src0 + q], y = Y[src0 + q], yaw = YAW[src0 + q];
      wx[q + shift] = (tc * x - ts * y) + tx;
      wy[q + shift] = (ts * x + tc * y) + ty;
      wyaw[q + shift] = tyaw == 0 ? yaw : normalize_theta(yaw + tyaw);
    }
  }
  __syncthreads();

  // ---- 6. via-points: a greedy chain over the transformed window, before its first pose is replaced ------------------------------------
  int nvia = 0;
  if (a.via_sep > 0 && W > 1 && fits) {
    if (wv == 0) {
      int prev = 0, cur = 1;
      while (cur < W) {
        const int j = cur + lane;
        bool acc = false;
        if (j < W) {
          const double ex = wx[j] - wx[prev], ey = wy[j] - wy[prev];
          acc = !(sqrt(ex * ex + ey * ey) < a.via_sep);
        }
        const unsigned long long m = __ballot(acc);
        if (m) {
          const int f = cur + __ffsll((long long)m) - 1;
          if (lane == 0) { vx[nvia] = wx[f]; vy[nvia] = wy[f]; }
          ++nvia; prev = f; cur = f + 1;
        } else {
          cur += 64;
        }
      }
      if (lane == 0) s_int[1] = nvia;
    }
    __syncthreads();
    nvia = pw_uniform(s_int[1]);
  }

  // ---- 7 / 8. the local goal, the start replacement, the transformed global goal: one lane ---------------------------------------------
  if (tid == 0) {
    const double gxp = X[N - 1], gyp = Y[N - 1], gyawp = YAW[N - 1];
    const double ggx = (tc * gxp - ts * gyp) + tx, ggy = (ts * gxp + tc * gyp) + ty;
    const double ggyaw = tyaw == 0 ? gyawp : normalize_theta(gyawp + tyaw);
    double lx, ly, lyaw;
    {
      const double x = X[goal_idx], y = Y[goal_idx], yaw = YAW[goal_idx];
      lx = (tc * x - ts * y) + tx; ly = (ts * x + tc * y) + ty;
      lyaw = tyaw == 0 ? yaw : normalize_theta(yaw + tyaw);
    }
    double goal_yaw = lyaw;
    if (a.overwrite_orientation) {
      int mal = a.moving_average_length;
      if (goal_idx > N - mal - 2) {
        goal_yaw = goal_idx >= N - 1 ? lyaw : ggyaw;
      } else {
        mal = mal < N - goal_idx - 1 ? mal : N - goal_idx - 1;
        double kx = lx, ky = ly, sc = 0.0, ss = 0.0;
        const int range_end = goal_idx + mal;
        for (int i = goal_idx; i < range_end; ++i) {
          const double x = X[i + 1], y = Y[i + 1];
          const double nx = (tc * x - ts * y) + tx, ny = (ts * x + tc * y) + ty;
          const double cand = atan2(ny - ky, nx - kx);
          sc += cos(cand); ss += sin(cand);
          if (i < range_end - 1) { kx = nx; ky = ny; }
        }
        goal_yaw = (sc == 0 && ss == 0) ? 0.0 : atan2(ss, sc);   // average_angles (misc.h:72-84)
      }
    }
    if (fits) {
      wyaw[W - 1 + shift] = goal_yaw;
      wx[0] = gx; wy[0] = gy; wyaw[0] = gth;   // transformed_plan.front() = robot_pose
    }
    out->window_count = W + shift; out->goal_idx = goal_idx; out->cursor = begin; out->pruned = pruned; out->via_count = nvia;
    out->alloc = A; out->off = off;
    out->goal[0] = lx; out->goal[1] = ly; out->goal[2] = goal_yaw;
    out->global_goal[0] = ggx; out->global_goal[1] = ggy; out->global_goal[2] = ggyaw;
    a.cursor[r] = begin;
  }
}

}  // namespace tebamd
