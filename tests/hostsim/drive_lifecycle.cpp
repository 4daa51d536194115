// drive_lifecycle.cpp -- driver (a) of the simulated runtime: a context's life and the growth of what it owns.
// create / destroy; nodes appended across the node capacity twice (grow_nodes, DevBuf::regrow); mirror edges appended
// across the edge capacity twice and the whole mirror read back (grow_edges); sphere lists of 0, 1, 40 and 1 500 and
// polygon lists of 0, 1 and 64 with and without paths, each used by a point and an edge check (the table blocks of
// block_layout.hpp go up in one transfer); an output array registered, used, unregistered and used again.  The obstacle
// group runs twice in the one context, the second time after a larger call has grown the workspaces.
#include "drive_common.hpp"

using namespace hostsim;

static void use_obstacles(rrtx_ctx *ctx, int kind, long long np, long long ne) {
  const int dim = scene.dim;
  Arr<double> p((size_t)np * dim), p0((size_t)ne * dim), p1((size_t)ne * dim), clr((size_t)np);
  fill_points(p, np, dim, 7); fill_points(p0, ne, dim, 11); fill_points(p1, ne, dim, 13);
  Arr<uint8_t> unsafe((size_t)np, 0x11), hit((size_t)ne, 0x11);
  Arr<int32_t> first((size_t)ne);
  OK(ctx, rrtx_points_check(ctx, kind, p, np, 0.1, 1, unsafe, clr));
  OK(ctx, rrtx_points_check(ctx, kind, p, np, 0.1, 0, unsafe, nullptr));
  OK(ctx, rrtx_edges_check(ctx, kind, p0, p1, ne, 0.1, -1, hit, first));
  long long missing = 0;
  for (long long i = 0; i < np; ++i) if (unsafe[i] == 0x11) ++missing;
  for (long long i = 0; i < ne; ++i) if (hit[i] == 0x11) ++missing;
  CHECK(missing == 0);
}

static void obstacle_group(rrtx_ctx *ctx, const char *pass) {
  for (int m : {0, 1, 40, 1500}) {
    fakehip::context(std::string(pass) + " spheres m=" + std::to_string(m));
    set_spheres(ctx, m);
    use_obstacles(ctx, 0, 5, 3);
    use_obstacles(ctx, 0, 300, 257);
  }
  for (int paths = 0; paths < 2; ++paths)
    for (int m : {0, 1, 64}) {
      fakehip::context(std::string(pass) + " polygons m=" + std::to_string(m) + (paths ? " with paths" : ""));
      set_polygons(ctx, m, paths != 0);
      use_obstacles(ctx, 1, 5, 3);
      use_obstacles(ctx, 1, 300, 257);      // (256 points and more: the grid over 64 obstacles and more)
    }
  // an output array of the caller's, registered with the context for straight DMA
  fakehip::context(std::string(pass) + " host_register");
  const long long ne = 1000;
  Arr<double> p0((size_t)ne * scene.dim), p1((size_t)ne * scene.dim);
  fill_points(p0, ne, scene.dim, 3); fill_points(p1, ne, scene.dim, 5);
  Arr<uint8_t> hit((size_t)ne, 0x11);
  OK(ctx, rrtx_edges_check(ctx, 0, p0, p1, ne, 0.1, -1, hit, nullptr));
  OK(ctx, rrtx_host_register(ctx, hit, (size_t)ne));
  OK(ctx, rrtx_host_register(ctx, hit, (size_t)ne));                 // (a range already registered: nothing to do)
  OK(ctx, rrtx_edges_check(ctx, 0, p0, p1, ne, 0.1, -1, hit, nullptr));
  OK(ctx, rrtx_host_unregister(ctx, hit));
  RC(ctx, RRTX_E_INVALID, rrtx_host_unregister(ctx, hit));
  OK(ctx, rrtx_edges_check(ctx, 0, p0, p1, ne, 0.1, -1, hit, nullptr));
}

int main() {
  register_contracts();
  rrtx_ctx *ctx = nullptr;
  fakehip::context("create");
  OK(nullptr, rrtx_create(&ctx, 3, 0, 1024));
  if (!ctx) return fakehip::report() | 1;
  scene = Scene{};

  // nodes across the capacity twice: 1024 -> 2048 -> 4096
  fakehip::context("nodes_append");
  for (long long n : {600, 600, 1, 1000, 0}) append_nodes(ctx, n);

  // edges across the capacity twice: 4096 -> 8192 -> 16384; then the whole mirror
  fakehip::context("graph_edges_append");
  long long ge = 0;
  for (long long n : {3000, 3000, 1, 4000}) {
    Arr<int32_t> s((size_t)n), e((size_t)n);
    for (long long i = 0; i < n; ++i) { s[i] = (int32_t)((ge + i) % scene.n_nodes); e[i] = (int32_t)((ge + i + 1) % scene.n_nodes); }
    int64_t first = -1;
    OK(ctx, rrtx_graph_edges_append(ctx, s, e, n, &first));
    CHECK(first == ge);
    ge += n;
  }
  CHECK(rrtx_graph_edges_count(ctx) == ge);
  {
    fakehip::context("graph_edges_get");
    Arr<int32_t> s((size_t)ge, -7), e((size_t)ge, -7);
    Arr<double> d((size_t)ge), d0((size_t)ge);
    OK(ctx, rrtx_graph_edges_get(ctx, nullptr, 0, ge, s, e, d, d0));
    // what was appended came through both regrows (the device-to-device copies of the kept part)
    long long wrong = 0;
    for (long long i = 0; i < ge; ++i) if (!(s[i] == (int32_t)(i % scene.n_nodes) && e[i] == (int32_t)((i + 1) % scene.n_nodes))) ++wrong;
    CHECK(wrong == 0);
    OK(ctx, rrtx_graph_edges_get(ctx, nullptr, ge - 1, 1, s, nullptr, nullptr, d0));
    RC(ctx, RRTX_E_INVALID, rrtx_graph_edges_get(ctx, nullptr, ge, 1, s, e, d, d0));
  }

  obstacle_group(ctx, "cold");
  // a larger call grows the staging workspaces and the outputs; then the same group again
  fakehip::context("larger call");
  set_spheres(ctx, 40);
  use_obstacles(ctx, 0, 70000, 70000);
  obstacle_group(ctx, "grown");

  fakehip::context("destroy");
  OK(ctx, rrtx_destroy(ctx));

  // a second context, [x y t theta]: its own allocations, nodes across the capacity, gone again
  fakehip::context("dim 4");
  scene = Scene{};
  scene.dim = 4;
  OK(nullptr, rrtx_create(&ctx, 4, 0, 0));
  for (long long n : {1000, 100}) append_nodes(ctx, n);
  OK(ctx, rrtx_destroy(ctx));
  return fakehip::report();
}
