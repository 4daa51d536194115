// drive_checks.cpp -- driver (b) of the simulated runtime: the stand-alone collision checks of the host-pointer form.
// rrtx_edges_check against spheres and polygons, rrtx_edges_check_idx with and without a mask, rrtx_points_check with
// and without the clearance, rrtx_simple_steer with either distance left out; with and without first_hit; with an obstacle range that is empty (the outputs are then
// cleared by memsets, zero_outputs).  Counts: 0, 1, 255, 256, 257; either side of the 256 KiB staging threshold for
// 4 * ne (65 536 / 65 537) and for ne (262 144 / 262 145); either side of a doubling of the staged endpoints'
// buffers, 8 * dim * ne = 4096 * 2^6, for dim 3 (10 922 / 10 923) and dim 4 (8 192 / 8 193); and 288 000.  Every count
// runs cold in rising order and again, falling, once the workspaces have grown.
#include "drive_common.hpp"

using namespace hostsim;

static const long long kCounts3[] = {0, 1, 255, 256, 257, 10922, 10923, 65536, 65537, 262144, 262145, 288000};
static const long long kCounts4[] = {1, 257, 8192, 8193};
constexpr int kInactive = 3;          // the obstacle of either list that is not in use: a range of it alone is empty

static void edges_case(rrtx_ctx *ctx, int kind, long long ne, bool want_first, bool empty_range) {
  const int dim = scene.dim;
  Arr<double> p0((size_t)ne * dim), p1((size_t)ne * dim);
  fill_points(p0, ne, dim, 1); fill_points(p1, ne, dim, 2);
  Arr<uint8_t> hit((size_t)ne, 0x11);
  Arr<int32_t> first((size_t)ne, 0x11111111);
  OK(ctx, rrtx_edges_check(ctx, kind, p0, p1, ne, 0.1, empty_range ? kInactive : -1, hit, want_first ? first.p : nullptr));
  // every byte of the outputs arrived; an empty range clears them
  long long missing = 0, not_cleared = 0;
  for (long long i = 0; i < ne; ++i) {
    if (hit[i] == 0x11 || (want_first && first[i] == 0x11111111)) ++missing;
    if (empty_range && !(hit[i] == 0 && (!want_first || first[i] == -1))) ++not_cleared;
  }
  CHECK(missing == 0);
  CHECK(not_cleared == 0);
}

static void idx_case(rrtx_ctx *ctx, long long ne, bool want_first, bool with_mask, bool empty_range) {
  Arr<int32_t> s((size_t)ne), e((size_t)ne);
  for (long long i = 0; i < ne; ++i) { s[i] = (int32_t)(i % scene.n_nodes); e[i] = (int32_t)((i * 7 + 1) % scene.n_nodes); }
  Arr<uint8_t> mask((size_t)scene.sph_na + 1, 1);      // one byte per sphere of the list, in list order
  Arr<uint8_t> hit((size_t)ne, 0x11);
  Arr<int32_t> first((size_t)ne, 0x11111111);
  OK(ctx, rrtx_edges_check_idx(ctx, s, e, ne, 0.1, empty_range ? kInactive : -1, with_mask ? mask.p : nullptr, hit,
                               want_first ? first.p : nullptr));
  // every byte of the outputs arrived; an empty range clears them
  long long missing = 0, not_cleared = 0;
  for (long long i = 0; i < ne; ++i) {
    if (hit[i] == 0x11 || (want_first && first[i] == 0x11111111)) ++missing;
    if (empty_range && !(hit[i] == 0 && (!want_first || first[i] == -1))) ++not_cleared;
  }
  CHECK(missing == 0);
  CHECK(not_cleared == 0);
}

static void points_case(rrtx_ctx *ctx, int kind, long long np, bool want_clearance, int quick) {
  const int dim = scene.dim;
  Arr<double> p((size_t)np * dim), clr((size_t)np, -77.0);
  fill_points(p, np, dim, 4);
  Arr<uint8_t> unsafe((size_t)np, 0x11);
  OK(ctx, rrtx_points_check(ctx, kind, p, np, 0.1, quick, unsafe, want_clearance ? clr.p : nullptr));
  long long missing = 0;
  for (long long i = 0; i < np; ++i) if (unsafe[i] == 0x11 || (want_clearance && clr[i] == -77.0)) ++missing;
  CHECK(missing == 0);
}

static void steer_case(rrtx_ctx *ctx, long long ne, bool want_dist, bool want_wdist) {
  const int dim = scene.dim;
  Arr<double> s((size_t)ne * dim), g((size_t)ne * dim), dist((size_t)ne, -77.0), wdist((size_t)ne, -77.0);
  fill_points(s, ne, dim, 5); fill_points(g, ne, dim, 6);
  OK(ctx, rrtx_simple_steer(ctx, s, g, ne, want_dist ? dist.p : nullptr, want_wdist ? wdist.p : nullptr));
  long long wrong = 0;
  for (long long i = 0; i < ne; ++i) if ((dist[i] != -77.0) != want_dist || (wdist[i] != -77.0) != want_wdist) ++wrong;
  CHECK(wrong == 0);
}

static void group(rrtx_ctx *ctx, const char *pass, long long n, bool polygons) {
  const std::string at = std::string(pass) + " dim=" + std::to_string(scene.dim) + " n=" + std::to_string(n);
  fakehip::context(at + " simple_steer");
  steer_case(ctx, n, true, true);
  if (n <= 10923) {                       // (an output left out changes no size: the small counts are enough)
    steer_case(ctx, n, true, false);
    steer_case(ctx, n, false, true);
  }
  // (first_hit and the empty range first: a buffer that has just grown is new, and its written shadow with it, so an
  // output that neither a kernel nor a memset writes shows there and nowhere later)
  for (int kind = 0; kind < (polygons ? 2 : 1); ++kind)
    for (int first = 1; first >= 0; --first)
      for (int empty = 1; empty >= 0; --empty) {
        fakehip::context(at + " edges_check kind=" + std::to_string(kind) + (first ? " first_hit" : "") + (empty ? " empty range" : ""));
        edges_case(ctx, kind, n, first != 0, empty != 0);
      }
  for (int first = 0; first < 2; ++first)
    for (int mask = 0; mask < 2; ++mask) {
      fakehip::context(at + " edges_check_idx" + (first ? " first_hit" : "") + (mask ? " mask" : ""));
      idx_case(ctx, n, first != 0, mask != 0, false);
    }
  fakehip::context(at + " edges_check_idx empty range");
  idx_case(ctx, n, true, true, true);
  for (int kind = 0; kind < (polygons ? 2 : 1); ++kind)
    for (int clr = 0; clr < 2; ++clr) {
      fakehip::context(at + " points_check kind=" + std::to_string(kind) + (clr ? " clearance" : ""));
      points_case(ctx, kind, n, clr != 0, clr);
    }
}

// the two obstacle lists, obstacle kInactive of each not in use
static void obstacles(rrtx_ctx *ctx, bool polygons) {
  const int m = 40;
  Arr<double> s(4 * (size_t)m);
  Arr<uint8_t> active((size_t)m, 1);
  active[kInactive] = 0;
  for (int i = 0; i < m; ++i) { for (int k = 0; k < 3; ++k) s[4 * i + k] = 10.0 * unit(i, 10 + k); s[4 * i + 3] = 0.2; }
  OK(ctx, rrtx_spheres_set(ctx, s, active, m));
  scene.sph_na = m - 1;
  if (!polygons) return;
  const int mp = 64;
  set_polygons(ctx, mp, false);
  int32_t which = kInactive;
  uint8_t off = 0;
  OK(ctx, rrtx_polygons_set_active(ctx, &which, 1, &off));
  scene.poly_na = mp - 1; scene.poly_nv = 4 * (mp - 1);
}

int main() {
  register_contracts();
  rrtx_ctx *ctx = nullptr;
  // the fourth report's call as its test makes it: the first and only call of a new context with no
  // node, 200 000 edges from pageable arrays, both distances wanted
  scene = Scene{};
  OK(nullptr, rrtx_create(&ctx, 3, 0, 0));
  if (!ctx) return fakehip::report() | 1;
  fakehip::context("first call: simple_steer of 200000");
  steer_case(ctx, 200000, true, true);
  OK(ctx, rrtx_destroy(ctx));

  scene = Scene{};
  OK(nullptr, rrtx_create(&ctx, 3, 0, 0));
  if (!ctx) return fakehip::report() | 1;
  append_nodes(ctx, 500);
  obstacles(ctx, true);
  for (long long n : kCounts3) group(ctx, "cold", n, true);
  for (int k = (int)(sizeof(kCounts3) / sizeof(kCounts3[0])) - 1; k >= 0; --k) group(ctx, "grown", kCounts3[k], true);
  OK(ctx, rrtx_destroy(ctx));

  // [x y t theta]: 32 bytes a staged point, so the endpoints' buffers double at other counts
  scene = Scene{};
  scene.dim = 4;
  OK(nullptr, rrtx_create(&ctx, 4, 0, 0));
  append_nodes(ctx, 500);
  obstacles(ctx, false);
  for (long long n : kCounts4) group(ctx, "cold", n, false);
  for (int k = (int)(sizeof(kCounts4) / sizeof(kCounts4[0])) - 1; k >= 0; --k) group(ctx, "grown", kCounts4[k], false);
  OK(ctx, rrtx_destroy(ctx));
  return fakehip::report();
}
