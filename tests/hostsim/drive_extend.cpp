// drive_extend.cpp -- driver (c) of the simulated runtime: rrtx_extend_candidates in a dim = 3 context, against the
// spheres and, with RRTX_OPT_EXTEND_OBSTACLES = 1, against the polygons (extend_csr_host: one block down, then the
// per-entry columns through the pinned arena or straight to the caller).
//
// The search runs on a tree of 600 nodes with the options as they come: below 8 192 nodes RRTX_OPT_NN_CULL = 1 leaves
// culling off, so launch_nn_radius takes the screened brute-force route -- pack, prep, scan, confirm, finish -- which
// needs five contracts and ONE script (the finish kernel's: it deals scene.total entries over the samples).  The culled
// route would need the slab index's kernels and the tile kernel as well.  RRTX_OPT_SCAN_BLOCKS = 8 keeps the scan's
// entry slices small; it changes no size the host form computes.
#include "drive_common.hpp"

using namespace hostsim;

struct Case {
  int nq; long long total, cap;
  bool needed = true, nearest = true, unsafe = true;
  int miss_every = 0;
};

static void extend_case(rrtx_ctx *ctx, const std::string &label, const Case &c) {
  fakehip::context(label + " nq=" + std::to_string(c.nq) + " total=" + std::to_string(c.total) + " cap=" + std::to_string(c.cap) +
                   (c.needed ? "" : " no needed") + (c.nearest ? "" : " no nearest") + (c.unsafe ? "" : " no sample_unsafe") +
                   (c.miss_every ? " nearest -1" : ""));
  scene.total = c.total;
  scene.nearest_miss_every = c.miss_every;
  const size_t nq = (size_t)c.nq, cap = (size_t)c.cap;
  Arr<double> q(3 * nq), cost(cap, -77.0), ndist(nq, -77.0);
  fill_points(q, c.nq, 3, 21);
  Arr<int64_t> offsets(nq + 1, -7);
  Arr<int32_t> idx(cap, 0x11111111), nidx(nq, 0x11111111);
  Arr<uint8_t> hit_out(cap, 0x11), hit_in(cap, 0x11), unsafe(nq, 0x11);
  int64_t needed = -7;
  const int rc = rrtx_extend_candidates(ctx, q, c.nq, 1.5, 0.1, offsets, idx, cost, hit_out, hit_in, c.cap,
                                        c.needed ? &needed : nullptr, c.nearest ? nidx.p : nullptr,
                                        c.nearest ? ndist.p : nullptr, c.unsafe ? unsafe.p : nullptr);
  if (c.nq == 0) { RC(ctx, RRTX_OK, rc); CHECK(offsets[0] == 0 && needed == 0); return; }
  const bool fits = c.total <= c.cap;
  RC(ctx, fits ? RRTX_OK : RRTX_E_CAPACITY, rc);
  if (c.needed) CHECK(needed == c.total);
  CHECK(offsets[0] == 0 && offsets[nq] == c.total);
  // the first `total` entries of every column arrived, and nothing beyond them (nothing at all when they do not fit)
  const size_t n_in = fits ? (size_t)c.total : 0;
  size_t bad = 0;
  for (size_t e = 0; e < cap; ++e) {
    const bool touched = idx[e] != 0x11111111, t2 = cost[e] != -77.0, t3 = hit_out[e] != 0x11, t4 = hit_in[e] != 0x11;
    if (e < n_in ? !(touched && cost[e] == 1.0 && hit_out[e] == 0 && hit_in[e] == 0) : (touched || t2 || t3 || t4)) ++bad;
    if (e < n_in && !(idx[e] >= 0 && idx[e] < scene.n_nodes)) ++bad;
  }
  CHECK(bad == 0);
  if (fits) {
    size_t bad_s = 0;
    for (size_t i = 0; i < nq; ++i) {
      if (c.nearest && !(nidx[i] >= 0 && nidx[i] < scene.n_nodes && ndist[i] == 1.0)) ++bad_s;   // (a -1 went to the fallback)
      if (c.unsafe && unsafe[i] != 0) ++bad_s;
    }
    CHECK(bad_s == 0);
  }
}

static void group(rrtx_ctx *ctx, const std::string &pass) {
  Case c;
  extend_case(ctx, pass, Case{0, 0, 0});
  extend_case(ctx, pass, Case{1, 5, 5});
  extend_case(ctx, pass, Case{1, 0, 0});                       // cap == 0 counts; nothing found
  extend_case(ctx, pass, Case{7, 30, 0});                      // cap == 0 counts: RRTX_E_CAPACITY with needed set
  // samples and block together beyond the arena's first MiB while the samples alone stay below it: the reservation of
  // the call has to count the block (a reservation short by it ends here, cold, as RRTX_E_NOMEM, "staging arena")
  extend_case(ctx, pass, Case{23300, 500, 500});
  extend_case(ctx, pass, Case{30000, 0, 0});
  // the samples on either side of the 1 MiB input threshold (3 * 8 * nq)
  extend_case(ctx, pass, Case{43690, 43690, 43690});
  extend_case(ctx, pass, Case{43691, 50000, 50000});
  // the entries so that each column lies on either side of 256 KiB: cost (8 bytes), idx (4), the flag bytes (1)
  for (long long total : {32768ll, 32769ll, 65536ll, 65537ll, 262144ll, 262145ll}) {
    extend_case(ctx, pass, Case{1000, total, total});          // total == cap
    extend_case(ctx, pass, Case{1000, total, total - 1});      // one more than fits: nothing is copied
  }
  extend_case(ctx, pass, Case{1000, 32768, 65537});            // room for more than was found
  extend_case(ctx, pass, Case{1000, 300, 262145});
  // outputs the caller did not ask for
  c = Case{500, 4000, 4000}; c.needed = false; extend_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.nearest = false; extend_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.unsafe = false; extend_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.needed = c.nearest = c.unsafe = false; extend_case(ctx, pass, c);
  // empty balls: a nearest index of -1 comes down and the host form asks the nearest search
  c = Case{500, 4000, 4000}; c.miss_every = 7; extend_case(ctx, pass, c);
  c = Case{3, 0, 8}; c.miss_every = 1; extend_case(ctx, pass, c);
  // small after large, large after small: the arena grows, and is used again
  extend_case(ctx, pass, Case{2, 6, 6});
  extend_case(ctx, pass, Case{43691, 262145, 262145});
  extend_case(ctx, pass, Case{2, 6, 6});
}

// The written shadow of a workspace outlives the call that wrote it, so a column no kernel writes shows only while the
// workspace is new: the calls without the optional outputs, each as the FIRST call of a context of its own.
static void first_call(const Case &c, int polygons) {
  rrtx_ctx *ctx = nullptr;
  scene = Scene{};
  OK(nullptr, rrtx_create(&ctx, 3, 0, 0));
  if (!ctx) return;
  OK(ctx, rrtx_set_option(ctx, RRTX_OPT_SCAN_BLOCKS, 8));
  OK(ctx, rrtx_set_option(ctx, RRTX_OPT_EXTEND_OBSTACLES, polygons));
  append_nodes(ctx, 600);
  set_spheres(ctx, 40);
  set_polygons(ctx, 64, false);
  // KNOWN: the per-sample block goes down whole, so the columns of outputs the caller did not ask for,
  // which no kernel then writes, travel as the workspace holds them.  The host form reads none of them (Field::to of a
  // null array, want_nearest), and every byte lies inside the block.  CandidatesBlock: offsets (nq + 1) and count, then
  // nearest_dist, nearest_idx, sample_unsafe: the first byte nothing wrote is the start of the first such column.
  const size_t csr_bytes = 8 * ((size_t)c.nq + 2);
  const bool whole = c.nearest && c.unsafe;
  if (!whole) fakehip::known_begin("first at offset " + std::to_string(c.nearest ? csr_bytes + 12 * (size_t)c.nq : csr_bytes) + " ");
  extend_case(ctx, polygons ? "first call, polygons" : "first call, spheres", c);
  if (!whole) fakehip::known_end();
  OK(ctx, rrtx_destroy(ctx));
}

int main() {
  register_contracts();
  for (int polygons = 0; polygons < 2; ++polygons)
    for (int k = 0; k < 5; ++k) {
      Case c{500, 4000, 4000};
      if (k == 1) c.needed = false;
      if (k == 2) c.nearest = false;
      if (k == 3) c.unsafe = false;
      if (k == 4) c.needed = c.nearest = c.unsafe = false;
      first_call(c, polygons);
    }
  rrtx_ctx *ctx = nullptr;
  scene = Scene{};
  OK(nullptr, rrtx_create(&ctx, 3, 0, 0));
  if (!ctx) return fakehip::report() | 1;
  OK(ctx, rrtx_set_option(ctx, RRTX_OPT_SCAN_BLOCKS, 8));
  append_nodes(ctx, 600);
  set_spheres(ctx, 40);
  set_polygons(ctx, 64, false);
  for (const char *pass : {"cold", "grown"})
    for (int polygons = 0; polygons < 2; ++polygons) {
      OK(ctx, rrtx_set_option(ctx, RRTX_OPT_EXTEND_OBSTACLES, polygons));
      group(ctx, std::string(pass) + (polygons ? " polygons" : " spheres"));
    }
  // polygons that move in time: the sample pass then takes the reference's loop, and the edge kernel its time column
  set_polygons(ctx, 64, true);
  extend_case(ctx, "moving polygons", Case{300, 2000, 2000});
  OK(ctx, rrtx_destroy(ctx));
  return fakehip::report();
}
