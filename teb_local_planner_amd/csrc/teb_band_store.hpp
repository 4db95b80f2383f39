// teb_band_store.hpp — ONE statement of "a set of bands" on the device: the strips of a set (BandStrips), the strips with the per-band
// attributes and results the kernels read through a BatchDev (DevBandStore), the attributes a band is born with (BandAttrs) and the
// layout of the packed messages small batches travel in. Plain C++ over include/teb_amd.h and DevBuf (teb_scene_store.hpp):
// tests/host/band_store_check.cpp compiles it alone with -DTEB_BAND_STORE_HOST_ONLY, over counting allocation primitives. The views are
// templates over the batch type, which is BatchDev (teb_device.hpp) wherever the library uses them.
#pragma once

#if defined(TEB_BAND_STORE_HOST_ONLY) && !defined(TEB_SCENE_STORE_HOST_ONLY)
#define TEB_SCENE_STORE_HOST_ONLY
#endif
#include <cstring>
#include <vector>

#include "teb_scene_store.hpp"   // DevBuf, AllocRun

namespace tebamd {

struct Strips { double *x, *y, *th, *dt; int* n; };   // the four strips of a set of bands and their pose counts

// The strips of `bands` bands: x, y, th, dt [bands x stride] and n [bands]. All five exist or none does.
struct BandStrips {
  DevBuf<double> x, y, th, dt;
  DevBuf<int> n;
  size_t bands() const { return n.n; }   // 0: not allocated

  DevError alloc(size_t count, size_t stride) {
    AllocRun A;
    A(x.alloc(count * stride)); A(y.alloc(count * stride)); A(th.alloc(count * stride)); A(dt.alloc(count * stride)); A(n.alloc(count));
    if (!A.ok()) free();
    return A.first;
  }
  void free() { *this = BandStrips(); }
  Strips view() const { return Strips{x.p, y.p, th.p, dt.p, n.p}; }
  // the strips seen as a batch of `bands` bands (the scratch strips candidates are initialised in)
  template <class Batch>
  void into(Batch& b) const { b.B = (int)bands(); b.n = n.p; b.x = x.p; b.y = y.p; b.th = th.p; b.dt = dt.p; }
};

// How long a column of a band store is: one entry per band, three per band (a velocity), one per pose.
enum class BandExtent { Band, Band3, Pose };

// THE column table of a band store beside its strips - what move_bands_kernel moves with attrs != 0, under the names of BatchDev:
// X(element type, name, extent, zeroed at create). The zeroed ones: "no statistics yet" for hasDiverged, optimized_ = false.
#define TEB_BAND_ATTR_COLUMNS(X)                                                                                                     \
  X(int, has_vs, Band, false) X(int, has_vg, Band, false) X(int, rotdir, Band, false) X(int, via_en, Band, false)                    \
  X(double, vs, Band3, false) X(double, vg, Band3, false)                                                                            \
  X(double, cost, Band, true) X(double, chi2, Band, true) X(int, iters, Band, true) X(int, last_iters, Band, true)                   \
  X(int, status, Band, true) X(int, optimized, Band, true) X(int, trials, Band, false) X(double, lambda, Band, false)

// f(column, its extent, zeroed at create) for the 19 columns of store s: the five of its strips, then the table above
template <class S, class F>
void for_each_band_column(S& s, F&& f) {
  f(s.strips.x, BandExtent::Pose, false); f(s.strips.y, BandExtent::Pose, false); f(s.strips.th, BandExtent::Pose, false);
  f(s.strips.dt, BandExtent::Pose, false); f(s.strips.n, BandExtent::Band, false);
#define TEB_BAND_VISIT(type, name, extent, zeroed) f(s.name, BandExtent::extent, zeroed);
  TEB_BAND_ATTR_COLUMNS(TEB_BAND_VISIT)
#undef TEB_BAND_VISIT
}

// The bands a BatchDev points at. A handle owns two: its live batch and, from the first compaction on, the scratch the bands are
// gathered through. All 19 columns exist or none does.
struct DevBandStore {
  BandStrips strips;
#define TEB_BAND_DECLARE(type, name, extent, zeroed) DevBuf<type> name;
  TEB_BAND_ATTR_COLUMNS(TEB_BAND_DECLARE)
#undef TEB_BAND_DECLARE

  bool allocated() const { return strips.bands() != 0; }
  DevError alloc(size_t bands, size_t stride) {
    AllocRun A;
    for_each_band_column(*this, [&](auto& c, BandExtent e, bool) {
      A(c.alloc(e == BandExtent::Band ? bands : e == BandExtent::Band3 ? 3 * bands : bands * stride));
    });
    if (!A.ok()) free();
    return A.first;
  }
  void free() { *this = DevBandStore(); }
  // zero(address, bytes) for every column that starts at zero, until one fails
  template <class Zero>
  DevError zero_at_create(Zero&& zero) {
    DevError err = kDevOk;
    for_each_band_column(*this, [&](auto& c, BandExtent, bool zeroed) {
      if (zeroed && err == kDevOk) err = zero(static_cast<void*>(c.p), c.n * sizeof(*c.p));
    });
    return err;
  }
  // the 19 pointers of b; B, the stride and the launch scratch stay the caller's
  template <class Batch>
  void view(Batch& b) const {
    b.n = strips.n.p; b.x = strips.x.p; b.y = strips.y.p; b.th = strips.th.p; b.dt = strips.dt.p;
#define TEB_BAND_POINT(type, name, extent, zeroed) b.name = name.p;
    TEB_BAND_ATTR_COLUMNS(TEB_BAND_POINT)
#undef TEB_BAND_POINT
  }
};

// ---- what a band is born with -------------------------------------------------------------------------------------------------------
struct BandAttrs {
  int has_vs, has_vg, rotdir, via_en, optimized;
  double vs[3], vg[3];
  // TebOptimalPlanner::initialize() (src/optimal_planner.cpp:86-104): start and goal velocity fixed at zero, no preferred rotation
  // direction, via-points on, optimized_ = false
  static BandAttrs fresh() { return BandAttrs{1, 1, TEB_AMD_ROT_NONE, 1, 0, {0, 0, 0}, {0, 0, 0}}; }
  // A band made from an exploration candidate (addAndInitNewTeb): setVelocityStart(start_vel), setVelocityGoalFree if asked for.
  // Born WITHOUT via-points - its constructor gets none; updateReferenceTrajectoryViaPoints switches them on after the tick.
  static BandAttrs candidate(const double* start_vel, int free_goal_vel) {
    BandAttrs a = fresh();
    a.via_en = 0;
    a.has_vg = free_goal_vel ? 0 : 1;
    if (start_vel) std::memcpy(a.vs, start_vel, sizeof a.vs);
    return a;
  }
};
// band b of the caller's batch: the caller's value where an optional array is given, fresh() where it is not
inline BandAttrs attrs_of(const teb_amd_teb_batch_t& bt, int b) {
  BandAttrs a = BandAttrs::fresh();
  if (bt.has_vel_start) a.has_vs = bt.has_vel_start[b] != 0;
  if (bt.has_vel_goal) a.has_vg = bt.has_vel_goal[b] != 0;
  if (bt.prefer_rotdir) a.rotdir = bt.prefer_rotdir[b];
  if (bt.via_points_enabled) a.via_en = bt.via_points_enabled[b] != 0;
  if (bt.vel_start) std::memcpy(a.vs, bt.vel_start + 3 * (size_t)b, sizeof a.vs);
  if (bt.vel_goal) std::memcpy(a.vg, bt.vel_goal + 3 * (size_t)b, sizeof a.vg);
  return a;
}
// the attributes of `count` bands as the arrays the columns are uploaded from
struct BandAttrArrays {
  std::vector<int> has_vs, has_vg, rotdir, via_en, optimized;
  std::vector<double> vs, vg;
  explicit BandAttrArrays(size_t count) : has_vs(count), has_vg(count), rotdir(count), via_en(count), optimized(count), vs(3 * count), vg(3 * count) {}
  void set(size_t k, const BandAttrs& a) {
    has_vs[k] = a.has_vs; has_vg[k] = a.has_vg; rotdir[k] = a.rotdir; via_en[k] = a.via_en; optimized[k] = a.optimized;
    std::memcpy(&vs[3 * k], a.vs, sizeof a.vs); std::memcpy(&vg[3 * k], a.vg, sizeof a.vg);
  }
};
inline BandAttrArrays attrs_of(const teb_amd_teb_batch_t& bt) {
  BandAttrArrays A((size_t)bt.count);
  for (int b = 0; b < bt.count; ++b) A.set((size_t)b, attrs_of(bt, b));
  return A;
}

// ---- the packed messages of small batches (doubles; the integer attributes are exact as doubles), host side of their layout ----------
// Upload (unpack_bands_kernel reads it): [n | has_vs | has_vg | rotdir | via_en] B each, [vs | vg] 3 B each, then x | y | theta | dt as
// planes of B rows of w columns. Download (pack_bands_kernel writes it): n [B], then the four planes.
struct UploadMsg {
  size_t B, w;
  size_t n() const { return 0; }
  size_t has_vs() const { return B; }   size_t has_vg() const { return 2 * B; }
  size_t rotdir() const { return 3 * B; }   size_t via_en() const { return 4 * B; }
  size_t vs() const { return 5 * B; }   size_t vg() const { return 8 * B; }
  size_t plane() const { return B * w; }
  size_t body(int k) const { return 11 * B + (size_t)k * plane(); }   // k = 0 .. 3: x, y, theta, dt
  size_t size() const { return body(4); }
};
struct DownloadMsg {
  size_t B, w;
  size_t n() const { return 0; }
  size_t plane() const { return B * w; }
  size_t body(int k) const { return B + (size_t)k * plane(); }
  size_t size() const { return body(4); }
};
// the caller's batch as an upload message of whole rows of w columns (the padding stays the caller's): m [UploadMsg{count, w}.size()]
inline void pack_upload(const teb_amd_teb_batch_t& bt, size_t w, double* m) {
  const UploadMsg L{(size_t)bt.count, w};
  const double* src[4] = {bt.x, bt.y, bt.theta, bt.dt};
  for (size_t b = 0; b < L.B; ++b) {
    const BandAttrs a = attrs_of(bt, (int)b);
    m[L.n() + b] = bt.n[b];
    m[L.has_vs() + b] = a.has_vs; m[L.has_vg() + b] = a.has_vg; m[L.rotdir() + b] = a.rotdir; m[L.via_en() + b] = a.via_en;
    for (int q = 0; q < 3; ++q) { m[L.vs() + 3 * b + q] = a.vs[q]; m[L.vg() + 3 * b + q] = a.vg[q]; }
    for (int k = 0; k < 4; ++k) std::memcpy(m + L.body(k) + b * w, src[k] + b * (size_t)bt.stride, w * sizeof(double));
  }
}
// ... and a download message into the caller's batch (n included)
inline void unpack_download(const double* m, size_t B, size_t w, teb_amd_teb_batch_t& bt) {
  const DownloadMsg L{B, w};
  double* dst[4] = {bt.x, bt.y, bt.theta, bt.dt};
  for (size_t b = 0; b < B; ++b) {
    for (int k = 0; k < 4; ++k) std::memcpy(dst[k] + b * (size_t)bt.stride, m + L.body(k) + b * w, w * sizeof(double));
    bt.n[b] = (int)m[L.n() + b];
  }
}

}  // namespace tebamd
