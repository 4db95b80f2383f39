// band_store_check.cpp — csrc/teb_band_store.hpp and the owner of device memory under it (DevBuf, csrc/teb_scene_store.hpp) on their
// own, without HIP: the two allocation primitives are defined HERE, over malloc, with a ledger of what is live and a switch that makes
// the k-th allocation fail. Ownership (every allocation freed exactly once), the all-or-none allocation of BandStrips and DevBandStore,
// their views, the defaults of a new band and the layout of the packed messages are checked against hand-written answers. Stand-alone:
// tests/test_band_store_host.py compiles it with the address and undefined-behaviour sanitizers (leak check on) and runs it; it prints
// what failed and returns the number of failures.
#define TEB_BAND_STORE_HOST_ONLY
#include "../../teb_local_planner_amd/csrc/teb_band_store.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>

using namespace tebamd;

static int g_failures = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failures; } \
  } while (0)

// ---- the counting primitives ----------------------------------------------------------------------------------------------------------
static std::map<void*, size_t> g_live;   // address -> bytes
static long g_allocs = 0, g_frees = 0, g_bad_frees = 0;
static long g_fail_at = -1;              // the allocation with this number (counted from 0 since arm()) fails; -1: none
static long g_since_arm = 0;
static void arm(long k) { g_fail_at = k; g_since_arm = 0; }

tebamd::DevError tebamd::device_allocate(void** p, size_t bytes) {
  if (g_since_arm++ == g_fail_at) { *p = nullptr; return 2; }   // (any code but 0)
  *p = std::malloc(bytes);
  g_live[*p] = bytes;
  ++g_allocs;
  return 0;
}
void tebamd::device_free(void* p) {
  if (g_live.erase(p) != 1) { ++g_bad_frees; return; }   // freed twice, or never allocated
  std::free(p);
  ++g_frees;
}

// a batch with the members of BatchDev (teb_device.hpp needs HIP; the views are templates over the batch type)
struct Batch {
  int B, stride;
  int* n;
  double *x, *y, *th, *dt;
  const int* has_vs; const double* vs; const int* has_vg; const double* vg; const int* rotdir; const int* via_en;
  int *status, *optimized, *iters, *last_iters, *trials;
  double *chi2, *cost, *lambda;
};

static void check_ownership() {
  const long a0 = g_allocs, f0 = g_frees;
  {   // scope exit
    DevBuf<double> b;
    CHECK(b.alloc(10) == 0 && b.p && b.n == 10);
    CHECK(g_live.at(b.p) == 10 * sizeof(double));
  }
  CHECK(g_allocs - a0 == 1 && g_frees - f0 == 1 && g_live.empty());
  {   // alloc(0): one element, so that p is an address
    DevBuf<int> z;
    CHECK(z.alloc(0) == 0 && z.p && z.n == 0 && g_live.at(z.p) == sizeof(int));
  }
  {   // move construction: the source is empty and frees nothing
    DevBuf<int> a;
    CHECK(a.alloc(4) == 0);
    int* was = a.p;
    DevBuf<int> b(std::move(a));
    CHECK(b.p == was && b.n == 4 && a.p == nullptr && a.n == 0);
    CHECK(g_live.size() == 1);
  }
  CHECK(g_live.empty() && g_allocs - a0 == 3 && g_frees - f0 == 3);
  {   // move assignment onto a live buffer frees the target first
    DevBuf<int> a, b;
    CHECK(a.alloc(4) == 0 && b.alloc(8) == 0);
    int *pa = a.p, *pb = b.p;
    b = std::move(a);
    CHECK(b.p == pa && b.n == 4 && a.p == nullptr && a.n == 0);
    CHECK(g_live.count(pb) == 0 && g_live.size() == 1);
  }
  CHECK(g_live.empty() && g_allocs - a0 == 5 && g_frees - f0 == 5);
  {   // alloc over a live buffer frees it first; a failed alloc leaves the buffer empty
    DevBuf<double> b;
    CHECK(b.alloc(3) == 0);
    double* first = b.p;
    CHECK(b.alloc(5) == 0 && b.n == 5);
    CHECK(g_live.count(first) == 0 && g_live.size() == 1);
    arm(0);
    CHECK(b.alloc(7) != 0 && b.p == nullptr && b.n == 0 && g_live.empty());
    arm(-1);
    b.free();   // (an empty buffer frees nothing)
    CHECK(b.alloc(2) == 0 && b.n == 2);
  }
  CHECK(g_live.empty() && g_allocs - a0 == 8 && g_frees - f0 == 8);
  {   // ensure: grows (the old block goes), does not shrink, does not touch a buffer that is large enough
    DevBuf<int> b;
    CHECK(ensure(b, 4) == 0 && b.n == 4);
    int* first = b.p;
    CHECK(ensure(b, 4) == 0 && b.p == first);
    CHECK(ensure(b, 2) == 0 && b.p == first && b.n == 4);
    CHECK(ensure(b, 9) == 0 && b.n == 9 && g_live.count(first) == 0 && g_live.size() == 1);
    arm(0);
    CHECK(ensure(b, 20) != 0 && b.p == nullptr && b.n == 0);   // a failed growth leaves nothing, and the next call allocates
    arm(-1);
    CHECK(ensure(b, 20) == 0 && b.n == 20);
  }
  CHECK(g_live.empty() && g_allocs - a0 == 11 && g_frees - f0 == 11 && g_bad_frees == 0);
}

// the k-th allocation of alloc() fails, for every k: nothing stays allocated, and a second alloc succeeds
template <class Store>
static void check_all_or_none(int columns) {
  for (int k = 0; k < columns; ++k) {
    Store s;
    arm(k);
    CHECK(s.alloc(5, 12) != 0);
    arm(-1);
    CHECK(g_live.empty());
    CHECK(s.alloc(5, 12) == 0);
    CHECK((int)g_live.size() == columns);
  }
  CHECK(g_live.empty() && g_bad_frees == 0);
  Store s;
  arm(columns);   // (one more than alloc() makes: it succeeds)
  CHECK(s.alloc(5, 12) == 0);
  arm(-1);
}

static void check_strips() {
  check_all_or_none<BandStrips>(5);
  BandStrips s;
  CHECK(s.bands() == 0 && s.view().x == nullptr);
  CHECK(s.alloc(5, 12) == 0 && s.bands() == 5);
  // [bands x stride] doubles four times, [bands] ints
  CHECK(s.x.n == 60 && s.y.n == 60 && s.th.n == 60 && s.dt.n == 60 && s.n.n == 5);
  CHECK(g_live.at(s.x.p) == 60 * sizeof(double) && g_live.at(s.n.p) == 5 * sizeof(int));
  const Strips v = s.view();
  CHECK(v.x == s.x.p && v.y == s.y.p && v.th == s.th.p && v.dt == s.dt.p && v.n == s.n.p);
  Batch b{};
  b.stride = 12;
  int other = 0;
  b.status = &other;
  s.into(b);
  CHECK(b.B == 5 && b.stride == 12 && b.n == s.n.p && b.x == s.x.p && b.y == s.y.p && b.th == s.th.p && b.dt == s.dt.p);
  CHECK(b.status == &other && b.has_vs == nullptr);   // into() writes the five pointers and B, nothing else
  BandStrips t(std::move(s));
  CHECK(s.view().x == nullptr && t.view().x == v.x && g_live.size() == 5);
  t.free();
  CHECK(t.bands() == 0 && g_live.empty());
}

static void check_store() {
  check_all_or_none<DevBandStore>(19);
  DevBandStore s;
  CHECK(!s.allocated());
  CHECK(s.alloc(5, 12) == 0 && s.allocated());
  // the column table: per pose
  CHECK(s.strips.x.n == 60 && s.strips.y.n == 60 && s.strips.th.n == 60 && s.strips.dt.n == 60);
  // per band
  CHECK(s.strips.n.n == 5 && s.has_vs.n == 5 && s.has_vg.n == 5 && s.rotdir.n == 5 && s.via_en.n == 5 && s.status.n == 5 && s.optimized.n == 5 &&
        s.iters.n == 5 && s.last_iters.n == 5 && s.trials.n == 5 && s.chi2.n == 5 && s.cost.n == 5 && s.lambda.n == 5);
  // three per band
  CHECK(s.vs.n == 15 && s.vg.n == 15);
  int columns = 0, per_band = 0, per_band3 = 0, per_pose = 0, zeroed = 0;
  for_each_band_column(s, [&](auto& c, BandExtent e, bool z) {
    ++columns; per_band += e == BandExtent::Band; per_band3 += e == BandExtent::Band3; per_pose += e == BandExtent::Pose; zeroed += z;
    CHECK(g_live.at(c.p) == c.n * sizeof(*c.p));
  });
  CHECK(columns == 19 && per_band == 13 && per_band3 == 2 && per_pose == 4 && zeroed == 6);
  // the view: every one of the 19 pointers at its own buffer, no two the same; B, the stride and nothing else touched
  Batch b{};
  b.B = 3; b.stride = 12;
  s.view(b);
  CHECK(b.B == 3 && b.stride == 12);
  CHECK(b.n == s.strips.n.p && b.x == s.strips.x.p && b.y == s.strips.y.p && b.th == s.strips.th.p && b.dt == s.strips.dt.p);
  CHECK(b.has_vs == s.has_vs.p && b.vs == s.vs.p && b.has_vg == s.has_vg.p && b.vg == s.vg.p && b.rotdir == s.rotdir.p && b.via_en == s.via_en.p);
  CHECK(b.status == s.status.p && b.optimized == s.optimized.p && b.iters == s.iters.p && b.last_iters == s.last_iters.p && b.trials == s.trials.p);
  CHECK(b.chi2 == s.chi2.p && b.cost == s.cost.p && b.lambda == s.lambda.p);
  const std::set<const void*> distinct{b.n, b.x, b.y, b.th, b.dt, b.has_vs, b.vs, b.has_vg, b.vg, b.rotdir, b.via_en, b.status, b.optimized, b.iters,
                                       b.last_iters, b.trials, b.chi2, b.cost, b.lambda};
  CHECK(distinct.size() == 19 && distinct.count(nullptr) == 0);
  // zeroed at create: cost, chi2, iters, last_iters, status, optimized - whole columns, in this order - and no other
  std::vector<std::pair<void*, size_t>> z;
  CHECK(s.zero_at_create([&](void* p, size_t bytes) { z.push_back({p, bytes}); return 0; }) == 0);
  const std::vector<std::pair<void*, size_t>> want{{s.cost.p, 5 * sizeof(double)}, {s.chi2.p, 5 * sizeof(double)}, {s.iters.p, 5 * sizeof(int)},
                                                   {s.last_iters.p, 5 * sizeof(int)}, {s.status.p, 5 * sizeof(int)}, {s.optimized.p, 5 * sizeof(int)}};
  CHECK(z == want);
  z.clear();
  CHECK(s.zero_at_create([&](void* p, size_t bytes) { z.push_back({p, bytes}); return z.size() == 2 ? 7 : 0; }) == 7 && z.size() == 2);   // stops at a failure
  DevBandStore t;
  t = std::move(s);
  CHECK(!s.allocated() && t.allocated() && g_live.size() == 19);
  t.free();
  CHECK(!t.allocated() && g_live.empty() && g_bad_frees == 0);
}

static bool same(const BandAttrs& a, int has_vs, int has_vg, int rotdir, int via_en, int optimized, double vs0, double vs1, double vs2, double vg0,
                 double vg1, double vg2) {
  return a.has_vs == has_vs && a.has_vg == has_vg && a.rotdir == rotdir && a.via_en == via_en && a.optimized == optimized && a.vs[0] == vs0 &&
         a.vs[1] == vs1 && a.vs[2] == vs2 && a.vg[0] == vg0 && a.vg[1] == vg1 && a.vg[2] == vg2;
}

static void check_defaults() {
  // TebOptimalPlanner::initialize(): both velocities fixed at zero, no preferred rotation direction (1), via-points on, not optimised
  const BandAttrs f = BandAttrs::fresh();
  CHECK(f.has_vs == 1); CHECK(f.has_vg == 1); CHECK(f.rotdir == 1 && TEB_AMD_ROT_NONE == 1); CHECK(f.via_en == 1); CHECK(f.optimized == 0);
  CHECK(f.vs[0] == 0 && f.vs[1] == 0 && f.vs[2] == 0); CHECK(f.vg[0] == 0 && f.vg[1] == 0 && f.vg[2] == 0);
  // a candidate: without via-points; the start velocity of its planner if there is one; a free goal velocity if asked for
  const double sv[3] = {0.25, -0.5, 0.125};
  CHECK(same(BandAttrs::candidate(nullptr, 0), 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0));
  CHECK(same(BandAttrs::candidate(nullptr, 1), 1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0));
  CHECK(same(BandAttrs::candidate(sv, 0), 1, 1, 1, 0, 0, 0.25, -0.5, 0.125, 0, 0, 0));
  CHECK(same(BandAttrs::candidate(sv, 1), 1, 0, 1, 0, 0, 0.25, -0.5, 0.125, 0, 0, 0));
  // attrs_of: each optional array present, one at a time (band 1 of 2), the others absent
  int32_t n[2] = {2, 2};
  double xs[4] = {0, 0, 0, 0};
  const int32_t flag[2] = {1, 0}, truthy[2] = {0, 5}, rot[2] = {TEB_AMD_ROT_NONE, TEB_AMD_ROT_RIGHT};
  const double vel[6] = {9, 9, 9, 1.5, 2.5, 3.5};
  teb_amd_teb_batch_t none{};
  none.count = 2; none.stride = 2; none.n = n; none.x = xs; none.y = xs; none.theta = xs; none.dt = xs;
  CHECK(same(attrs_of(none, 0), 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0) && same(attrs_of(none, 1), 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0));
  teb_amd_teb_batch_t b = none;
  b.has_vel_start = flag;
  CHECK(same(attrs_of(b, 1), 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0) && same(attrs_of(b, 0), 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0));
  b.has_vel_start = truthy;   // (any non-zero value is 1)
  CHECK(attrs_of(b, 1).has_vs == 1 && attrs_of(b, 0).has_vs == 0);
  b = none; b.has_vel_goal = flag;
  CHECK(same(attrs_of(b, 1), 1, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0));
  b = none; b.prefer_rotdir = rot;
  CHECK(same(attrs_of(b, 1), 1, 1, 2, 1, 0, 0, 0, 0, 0, 0, 0) && attrs_of(b, 0).rotdir == 1);
  b = none; b.via_points_enabled = flag;
  CHECK(same(attrs_of(b, 1), 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0) && attrs_of(b, 0).via_en == 1);
  b = none; b.vel_start = vel;
  CHECK(same(attrs_of(b, 1), 1, 1, 1, 1, 0, 1.5, 2.5, 3.5, 0, 0, 0));
  b = none; b.vel_goal = vel;
  CHECK(same(attrs_of(b, 1), 1, 1, 1, 1, 0, 0, 0, 0, 1.5, 2.5, 3.5));
  // the array forms
  b = none; b.has_vel_goal = flag; b.vel_start = vel;
  const BandAttrArrays A = attrs_of(b);
  CHECK((A.has_vs == std::vector<int>{1, 1}) && (A.has_vg == std::vector<int>{1, 0}) && (A.rotdir == std::vector<int>{1, 1}) &&
        (A.via_en == std::vector<int>{1, 1}) && (A.optimized == std::vector<int>{0, 0}));
  CHECK((A.vs == std::vector<double>{9, 9, 9, 1.5, 2.5, 3.5}) && (A.vg == std::vector<double>(6, 0.0)));
  BandAttrArrays C(2);
  C.set(1, BandAttrs::candidate(sv, 1));
  CHECK((C.has_vs == std::vector<int>{0, 1}) && (C.has_vg == std::vector<int>{0, 0}) && (C.rotdir == std::vector<int>{0, 1}) &&
        (C.via_en == std::vector<int>{0, 0}) && (C.vs == std::vector<double>{0, 0, 0, 0.25, -0.5, 0.125}));
}

static void check_messages() {
  // 3 bands of 2, 5 and 5 poses in rows of 5: pose i of band b is x = 100 b + i, y = x + 0.25, theta = x + 0.5, dt = x + 0.75
  int32_t n[3] = {2, 5, 5};
  double x[15], y[15], th[15], dt[15];
  for (int b = 0; b < 3; ++b)
    for (int i = 0; i < 5; ++i) { x[5 * b + i] = 100 * b + i; y[5 * b + i] = 100 * b + i + 0.25; th[5 * b + i] = 100 * b + i + 0.5; dt[5 * b + i] = 100 * b + i + 0.75; }
  const int32_t hvs[3] = {1, 0, 1}, rot[3] = {TEB_AMD_ROT_NONE, TEB_AMD_ROT_LEFT, TEB_AMD_ROT_RIGHT};
  const double vs[9] = {0.1, 0.2, 0.3, 1.1, 1.2, 1.3, 2.1, 2.2, 2.3};
  teb_amd_teb_batch_t bt{};
  bt.count = 3; bt.stride = 5; bt.n = n; bt.x = x; bt.y = y; bt.theta = th; bt.dt = dt;
  bt.has_vel_start = hvs; bt.prefer_rotdir = rot; bt.vel_start = vs;   // has_vel_goal, via_points_enabled, vel_goal: absent
  const UploadMsg L{3, 5};
  CHECK(L.n() == 0 && L.has_vs() == 3 && L.has_vg() == 6 && L.rotdir() == 9 && L.via_en() == 12 && L.vs() == 15 && L.vg() == 24);
  CHECK(L.plane() == 15 && L.body(0) == 33 && L.body(1) == 48 && L.body(2) == 63 && L.body(3) == 78 && L.size() == 93);
  const double want[93] = {
      2, 5, 5,                                         // n
      1, 0, 1,                                         // has_vs
      1, 1, 1,                                         // has_vg
      1, 0, 2,                                         // rotdir
      1, 1, 1,                                         // via_en
      0.1, 0.2, 0.3, 1.1, 1.2, 1.3, 2.1, 2.2, 2.3,     // vs
      0, 0, 0, 0, 0, 0, 0, 0, 0,                       // vg
      0, 1, 2, 3, 4, 100, 101, 102, 103, 104, 200, 201, 202, 203, 204,                                                          // x
      0.25, 1.25, 2.25, 3.25, 4.25, 100.25, 101.25, 102.25, 103.25, 104.25, 200.25, 201.25, 202.25, 203.25, 204.25,             // y
      0.5, 1.5, 2.5, 3.5, 4.5, 100.5, 101.5, 102.5, 103.5, 104.5, 200.5, 201.5, 202.5, 203.5, 204.5,                            // theta
      0.75, 1.75, 2.75, 3.75, 4.75, 100.75, 101.75, 102.75, 103.75, 104.75, 200.75, 201.75, 202.75, 203.75, 204.75};            // dt
  std::vector<double> m(L.size() + 1, -7.0);
  pack_upload(bt, 5, m.data());
  for (size_t k = 0; k < 93; ++k)
    if (m[k] != want[k]) { std::printf("FAILED upload message word %zu: %g, expected %g\n", k, m[k], want[k]); ++g_failures; }
  CHECK(m[93] == -7.0);   // nothing past the message
  // rows narrower than the caller's stride (the handle holds fewer poses): whole rows of w columns
  const UploadMsg N{3, 2};
  CHECK(N.body(0) == 33 && N.plane() == 6 && N.size() == 57);
  std::vector<double> q(N.size(), -7.0);
  pack_upload(bt, 2, q.data());
  const double xw[6] = {0, 1, 100, 101, 200, 201}, dw[6] = {0.75, 1.75, 100.75, 101.75, 200.75, 201.75};
  for (int k = 0; k < 6; ++k) CHECK(q[N.body(0) + k] == xw[k] && q[N.body(3) + k] == dw[k]);
  // the download message: n [B], then the four planes
  const DownloadMsg D{3, 5};
  CHECK(D.n() == 0 && D.plane() == 15 && D.body(0) == 3 && D.body(1) == 18 && D.body(2) == 33 && D.body(3) == 48 && D.size() == 63);
  std::vector<double> d(D.size());
  for (size_t k = 0; k < d.size(); ++k) d[k] = 1000.0 + (double)k;
  d[0] = 4; d[1] = 2; d[2] = 5;
  int32_t on[4] = {-1, -1, -1, -1};
  double ox[28], oy[28], oth[28], odt[28];   // a caller's batch of 4 rows of stride 7
  for (int k = 0; k < 28; ++k) ox[k] = oy[k] = oth[k] = odt[k] = -1;
  teb_amd_teb_batch_t out{};
  out.count = 4; out.stride = 7; out.n = on; out.x = ox; out.y = oy; out.theta = oth; out.dt = odt;
  unpack_download(d.data(), 3, 5, out);
  CHECK(on[0] == 4 && on[1] == 2 && on[2] == 5 && on[3] == -1);
  for (int b = 0; b < 3; ++b)
    for (int i = 0; i < 7; ++i) {
      const int at = 7 * b + i, k = 5 * b + i;
      if (i < 5) CHECK(ox[at] == 1003 + k && oy[at] == 1018 + k && oth[at] == 1033 + k && odt[at] == 1048 + k);
      else CHECK(ox[at] == -1 && oy[at] == -1 && oth[at] == -1 && odt[at] == -1);   // the padding stays the caller's
    }
  for (int k = 21; k < 28; ++k) CHECK(ox[k] == -1 && odt[k] == -1);
}

int main() {
  check_ownership();
  check_strips();
  check_store();
  check_defaults();
  check_messages();
  CHECK(g_live.empty());
  CHECK(g_allocs == g_frees);
  CHECK(g_bad_frees == 0);
  if (g_failures == 0) std::printf("band store check ok (%ld allocations, each freed once)\n", g_allocs);
  return g_failures;
}
