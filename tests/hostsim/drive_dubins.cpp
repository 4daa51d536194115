// drive_dubins.cpp -- driver (d) of the simulated runtime: rrtx_extend_candidates_dubins, the host form that still runs
// on stage_in / copy_out / read_count with a layout of its own (three double columns, two word columns of three bytes
// an entry, the flag bytes and sample_unsafe in ONE byte workspace of 8 * cap + nq).  Two dim = 4 contexts: without
// wrapped dimensions (the nearest node comes off the lists, and a -1 goes to the fallback) and with theta wrapped
// (every query has a ghost, and the nearest search runs as launches of its own).  The search takes the screened
// brute-force route as in drive_extend.cpp; the candidate edges add a steering and two check launches a chunk.
#include "drive_common.hpp"

using namespace hostsim;

struct Case {
  int nq; long long total, cap;
  bool needed = true, nearest = true, unsafe = true, words = true;
  int miss_every = 0;
};

static void dubins_case(rrtx_ctx *ctx, const std::string &label, const Case &c) {
  fakehip::context(label + " nq=" + std::to_string(c.nq) + " total=" + std::to_string(c.total) + " cap=" + std::to_string(c.cap) +
                   (c.needed ? "" : " no needed") + (c.nearest ? "" : " no nearest") + (c.unsafe ? "" : " no sample_unsafe") +
                   (c.words ? "" : " no words") + (c.miss_every ? " nearest -1" : ""));
  scene.total = c.total;
  scene.nearest_miss_every = c.miss_every;
  const size_t nq = (size_t)c.nq, cap = (size_t)c.cap;
  Arr<double> q(4 * nq), key(cap, -77.0), cost_out(cap, -77.0), cost_in(cap, -77.0), ndist(nq, -77.0);
  fill_points(q, c.nq, 4, 31);
  Arr<int64_t> offsets(nq + 1, -7);
  Arr<int32_t> idx(cap, 0x11111111), nidx(nq, 0x11111111);
  Arr<uint8_t> word_out(3 * cap, 0x11), word_in(3 * cap, 0x11), hit_out(cap, 0x11), hit_in(cap, 0x11), unsafe(nq, 0x11);
  int64_t needed = -7;
  const int rc = rrtx_extend_candidates_dubins(ctx, q, c.nq, 1.5, 0.1, 0.5, offsets, idx, key, cost_out, cost_in,
                                               c.words ? word_out.p : nullptr, c.words ? word_in.p : nullptr, hit_out, hit_in,
                                               c.cap, c.needed ? &needed : nullptr, c.nearest ? nidx.p : nullptr,
                                               c.nearest ? ndist.p : nullptr, c.unsafe ? unsafe.p : nullptr);
  if (c.nq == 0) { RC(ctx, RRTX_OK, rc); CHECK(offsets[0] == 0 && needed == 0); return; }
  const bool fits = c.total <= c.cap;
  RC(ctx, fits ? RRTX_OK : RRTX_E_CAPACITY, rc);
  if (c.needed) CHECK(needed == c.total);
  CHECK(offsets[0] == 0 && offsets[nq] == c.total);
  const size_t n_in = fits ? (size_t)c.total : 0;
  size_t bad = 0;
  for (size_t e = 0; e < cap; ++e) {
    const bool in = e < n_in;
    if ((idx[e] != 0x11111111) != in || (key[e] != -77.0) != in || (cost_out[e] != -77.0) != in || (cost_in[e] != -77.0) != in) ++bad;
    if (in ? !(hit_out[e] == 0 && hit_in[e] == 0) : !(hit_out[e] == 0x11 && hit_in[e] == 0x11)) ++bad;
    for (int k = 0; k < 3; ++k) {
      const bool w = word_out[3 * e + k] != 0x11, w2 = word_in[3 * e + k] != 0x11;
      if (w != (in && c.words) || w2 != (in && c.words)) ++bad;
    }
  }
  CHECK(bad == 0);
  if (fits) {
    size_t bad_s = 0;
    for (size_t i = 0; i < nq; ++i) {
      if (c.nearest && !(nidx[i] >= 0 && nidx[i] < scene.n_nodes && ndist[i] == 1.0)) ++bad_s;
      if (c.unsafe && unsafe[i] != 0) ++bad_s;
    }
    CHECK(bad_s == 0);
  }
}

// large: the cases whose workspaces run to hundreds of megabytes here (128 bytes of steering record an entry and
// direction; with a ghost a query, 16 KB of candidate records a copy in the nearest search): once, in the plain context
static void group(rrtx_ctx *ctx, const std::string &pass, bool large) {
  Case c;
  dubins_case(ctx, pass, Case{0, 0, 0});
  dubins_case(ctx, pass, Case{1, 5, 5});
  dubins_case(ctx, pass, Case{1, 0, 0});
  dubins_case(ctx, pass, Case{7, 30, 0});                      // cap == 0 counts
  // entries on either side of a doubling of each workspace: 8 * cap + nq bytes of flags and words, 4 * cap, 24 * cap
  for (long long total : {511ll, 512ll, 513ll, 1024ll, 1025ll, 4096ll, 4097ll, 65536ll, 65537ll, 262144ll, 262145ll}) {
    if (total > 100000 && !large) break;
    dubins_case(ctx, pass, Case{total < 1000 ? 100 : 1000, total, total});
    dubins_case(ctx, pass, Case{total < 1000 ? 100 : 1000, total, total - 1});   // one more than fits: nothing is copied
  }
  if (large) dubins_case(ctx, pass, Case{40000, 40000, 40000});   // many samples, one entry each
  dubins_case(ctx, pass, Case{1000, 300, 262145});              // room for far more than was found
  // outputs the caller did not ask for
  c = Case{500, 4000, 4000}; c.needed = false; dubins_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.nearest = false; dubins_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.unsafe = false; dubins_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.words = false; dubins_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.needed = c.nearest = c.unsafe = c.words = false; dubins_case(ctx, pass, c);
  c = Case{500, 4000, 4000}; c.miss_every = 7; dubins_case(ctx, pass, c);
  c = Case{3, 0, 8}; c.miss_every = 1; dubins_case(ctx, pass, c);
  dubins_case(ctx, pass, Case{2, 6, 6});
}

static void context_run(bool wrapped, bool space_has_time) {
  rrtx_ctx *ctx = nullptr;
  scene = Scene{};
  scene.dim = 4;
  OK(nullptr, rrtx_create(&ctx, 4, 0, 0));
  if (!ctx) return;
  OK(ctx, rrtx_set_option(ctx, RRTX_OPT_SCAN_BLOCKS, 8));
  if (wrapped) OK(ctx, rrtx_set_wrap(ctx, 3, 6.283185307179586));
  if (space_has_time) OK(ctx, rrtx_set_option(ctx, RRTX_OPT_SPACE_HAS_TIME, 1));
  append_nodes(ctx, 600);
  set_polygons(ctx, 64, false);
  const std::string what = std::string(wrapped ? "wrapped" : "plain") + (space_has_time ? " with time" : "");
  // the first call of the context without its optional outputs: what no kernel writes shows while the workspaces are new
  Case c{500, 4000, 4000};
  c.needed = c.nearest = c.unsafe = c.words = false;
  dubins_case(ctx, "first call, " + what, c);
  if (space_has_time) {                       // (the check kernel's build with time; the host form does nothing else)
    dubins_case(ctx, what, Case{100, 513, 513});
    dubins_case(ctx, what, Case{100, 513, 512});
    dubins_case(ctx, what, Case{1000, 65537, 65537});
    dubins_case(ctx, what, Case{2, 6, 6});
  } else {
    group(ctx, "cold " + what, !wrapped);
    if (!wrapped) group(ctx, "grown " + what, false);
  }
  OK(ctx, rrtx_destroy(ctx));
}

int main() {
  register_contracts();
  context_run(false, false);
  context_run(true, false);
  context_run(false, true);
  return fakehip::report();
}
