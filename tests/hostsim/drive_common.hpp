// drive_common.hpp -- what the drivers share: arrays of exactly the size the C-ABI asks for (pageable heap memory, so a
// write past a caller's array is the sanitizer's to catch), scenes, and the checked call.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/rrtx.h"
#include "contracts.hpp"
#include "fake_hip.hpp"

namespace hostsim {

template <class T>
struct Arr {
  T *p;
  size_t n;
  explicit Arr(size_t count, T fill = T()) : p(new T[count]), n(count) { for (size_t i = 0; i < n; ++i) p[i] = fill; }
  Arr(const Arr &) = delete;
  ~Arr() { delete[] p; }
  operator T *() const { return p; }
};

inline void expect_rc(rrtx_ctx *ctx, int got, int want, const char *expr, int line) {
  if (got != want)
    fakehip::finding("driver line %d: %s returned %d, not %d (%s)", line, expr, got, want,
                     ctx ? rrtx_last_error(ctx) : rrtx_create_error());
}
#define OK(ctx, expr) ::hostsim::expect_rc((ctx), (expr), RRTX_OK, #expr, __LINE__)
#define RC(ctx, want, expr) ::hostsim::expect_rc((ctx), (expr), (want), #expr, __LINE__)
#define CHECK(cond) do { if (!(cond)) fakehip::finding("driver line %d: %s does not hold", __LINE__, #cond); } while (0)

// a value in [0, 1) that depends on nothing but (i, k)
inline double unit(long long i, int k) {
  unsigned long long x = (unsigned long long)i * 0x9E3779B97F4A7C15ull + (unsigned long long)(k + 1) * 0xBF58476D1CE4E5B9ull;
  x ^= x >> 31; x *= 0x94D049BB133111EBull; x ^= x >> 29;
  return (double)(x >> 11) / 9007199254740992.0;
}
inline void fill_points(double *p, long long n, int dim, long long salt = 0) {
  for (long long i = 0; i < n; ++i)
    for (int k = 0; k < dim; ++k) p[i * dim + k] = 10.0 * unit(i + salt, k);
}

// m spheres (cx cy cz r), all in use
inline void set_spheres(rrtx_ctx *ctx, int m) {
  Arr<double> s(4 * (size_t)m);
  for (int i = 0; i < m; ++i) {
    for (int k = 0; k < 3; ++k) s[4 * i + k] = 10.0 * unit(i, 10 + k);
    s[4 * i + 3] = 0.05 + 0.2 * unit(i, 13);
  }
  OK(ctx, rrtx_spheres_set(ctx, s, nullptr, m));
  scene.sph_na = m;
}

// m square polygons; with paths: every fourth one moves in time (kind 6) along three rows of (dx, dy, t)
inline void set_polygons(rrtx_ctx *ctx, int m, bool paths) {
  Arr<int32_t> off((size_t)m + 1);
  Arr<double> vxy(8 * (size_t)m);
  Arr<uint8_t> kind((size_t)m, (uint8_t)3);
  for (int i = 0; i < m; ++i) {
    const double cx = 10.0 * unit(i, 20), cy = 10.0 * unit(i, 21), h = 0.1 + 0.2 * unit(i, 22);
    const double v[8] = {cx - h, cy - h, cx + h, cy - h, cx + h, cy + h, cx - h, cy + h};
    for (int k = 0; k < 8; ++k) vxy[8 * i + k] = v[k];
    off[i] = 4 * i;
    if (paths && i % 4 == 0) kind[i] = 6;
  }
  off[m] = 4 * m;
  OK(ctx, rrtx_polygons_set(ctx, off, vxy, nullptr, kind, nullptr, m));
  int rows = 0;
  if (paths) {
    Arr<int32_t> poff((size_t)m + 1);
    std::vector<double> path;
    for (int i = 0; i < m; ++i) {
      poff[i] = (int32_t)(path.size() / 3);
      if (kind[i] == 6)
        for (int k = 0; k < 3; ++k) { path.push_back(0.1 * k); path.push_back(0.05 * k); path.push_back((double)k); }
    }
    poff[m] = (int32_t)(path.size() / 3);
    rows = poff[m];
    Arr<double> pxyt(path.size());
    for (size_t k = 0; k < path.size(); ++k) pxyt[k] = path[k];
    OK(ctx, rrtx_polygon_paths_set(ctx, poff, pxyt, m));
  }
  scene.poly_na = m; scene.poly_nv = 4 * m; scene.poly_rows = rows;
}

inline void append_nodes(rrtx_ctx *ctx, long long n) {
  Arr<double> pos((size_t)n * scene.dim);
  fill_points(pos, n, scene.dim, scene.n_nodes);
  int64_t first = -1;
  OK(ctx, rrtx_nodes_append(ctx, pos, n, &first));
  CHECK(first == scene.n_nodes);
  scene.n_nodes += n;
  CHECK(rrtx_nodes_count(ctx) == scene.n_nodes);
}

}  // namespace hostsim
