// rrtx_capi.hip -- the extern "C" surface of librrtx_hip.so (include/rrtx.h):
// context lifetime, node/obstacle tables, host-buffer staging around the kernel
// launchers.  gfx950 only; no CPU fallback: every compute entry point runs HIP
// kernels or fails with RRTX_E_DEVICE.
#include <dlfcn.h>

#include <cstdarg>
#include <mutex>

#include "block_layout.hpp"
#include "exact_math.hpp"
#include "rrtx_internal.hpp"

namespace rrtx {

int fail(rrtx_ctx *ctx, int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (ctx) ctx->err = buf;
  return code;
}

// ---- roctx ranges around the C-ABI calls (tracing hook) ---------------------------------
// A rocprofv3 --marker-trace of a Julia-hosted run then shows which planner call every kernel belongs
// to.  The marker library is looked up at run time (rocprofiler-sdk's roctx, else the legacy one) so the
// library carries no link dependency on it; without it the ranges are no-ops.
namespace {
typedef int (*roctx_push_fn)(const char *);
typedef int (*roctx_pop_fn)(void);
roctx_push_fn g_roctx_push = nullptr;
roctx_pop_fn g_roctx_pop = nullptr;
std::once_flag g_roctx_once;
void roctx_resolve() {
  const char *names[] = {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"};
  for (const char *n : names) {
    void *h = dlopen(n, RTLD_LAZY | RTLD_GLOBAL);
    if (!h) continue;
    roctx_push_fn push = reinterpret_cast<roctx_push_fn>(dlsym(h, "roctxRangePushA"));
    roctx_pop_fn pop = reinterpret_cast<roctx_pop_fn>(dlsym(h, "roctxRangePop"));
    if (push && pop) { g_roctx_push = push; g_roctx_pop = pop; return; }
  }
}
}  // namespace

ApiRange::ApiRange(const char *name) {
  std::call_once(g_roctx_once, roctx_resolve);
  active = g_roctx_push != nullptr;
  if (active) (void)g_roctx_push(name);
}
ApiRange::~ApiRange() {
  if (active) (void)g_roctx_pop();
}

// ---- exact thresholds on squared distances (exact_math.hpp) -------------------
double thr_first_ge(double r) { return sq_first_ge(r); }
double thr_first_gt(double r) { return sq_first_gt(r); }

// first s with !((sqrt(s) - robotRadius) - radius < 0): explicitPointCheck's per-sphere test
// (R/DRRT_Q.jl:1555-1570) as a threshold on the squared distance, "collision <=> s < thr".
// The expression is monotone in s (every step is a monotone rounded operation).
double thr_point_clear(double robot_radius, double radius) {
  const double g = robot_radius + radius;
  double t = first_true(g * g, [=](double s) { return !((std::sqrt(s) - robot_radius) - radius < 0.0); });
  return std::isnan(t) ? INFINITY : t;      // never clear (e.g. infinite radius): s < +inf
}

// ---- profiling spans -------------------------------------------------------------
static hipEvent_t take_event(rrtx_ctx *ctx) {
  if (!ctx->event_pool.empty()) {
    hipEvent_t e = ctx->event_pool.back();
    ctx->event_pool.pop_back();
    return e;
  }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}

void span_begin(rrtx_ctx *ctx, int family) {
  ctx->fam_launches[family] += 1;
  // level 1 times only the dominant kernel family: every event record costs ~10 us of pipeline
  // drain between two kernels that would otherwise run back to back
  ctx->span_open = ctx->profiling == 2;
  if (ctx->profiling == 1 && family == KF_NN_SCAN) {
    // level 1 may sample: only every opt_profile_every-th launch of the family carries events
    ctx->span_tick += 1;
    ctx->span_open = ctx->span_tick % ctx->opt_profile_every == 0;
  }
  if (!ctx->span_open) { ctx->fam_launches[family] -= 1; return; }   // launches = timed launches
  TimedSpan s;
  s.a = take_event(ctx);
  s.b = take_event(ctx);
  s.family = family;
  (void)hipEventRecord(s.a, ctx->stream);
  ctx->spans.push_back(s);
}

void span_end(rrtx_ctx *ctx) {
  if (!ctx->span_open || ctx->spans.empty()) return;
  (void)hipEventRecord(ctx->spans.back().b, ctx->stream);
  ctx->span_open = false;
}

static void drain_spans(rrtx_ctx *ctx) {
  for (auto &s : ctx->spans) {
    float ms = 0.f;
    if (hipEventSynchronize(s.b) == hipSuccess && hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess)
      ctx->fam_ms[s.family] += ms;
    ctx->event_pool.push_back(s.a);
    ctx->event_pool.push_back(s.b);
  }
  ctx->spans.clear();
}

namespace {

// row-major points -> SoA.  fp64 arrays hold the coordinates as given; the fp32
// shadow (prefilter only) holds coordinates relative to the context origin plus
// |p~|^2, and absmax tracks max |p - origin| (bit pattern of a non-negative double
// orders like the value; NaN sorts above inf).
__global__ __launch_bounds__(256) void aos_to_soa_kernel(const double *__restrict__ pos, int dim, long long n,
                                                         long long base, double ox, double oy, double oz,
                                                         double ow, double *__restrict__ x,
                                                         double *__restrict__ y, double *__restrict__ z,
                                                         double *__restrict__ w, float *__restrict__ xf,
                                                         float *__restrict__ yf, float *__restrict__ zf,
                                                         float *__restrict__ wf, float *__restrict__ ppf,
                                                         unsigned long long *__restrict__ absmax,
                                                         float *__restrict__ sx, float *__restrict__ sy,
                                                         float *__restrict__ sz, float *__restrict__ sw,
                                                         float *__restrict__ spp, int32_t *__restrict__ sid,
                                                         double *__restrict__ dx, double *__restrict__ dy,
                                                         double *__restrict__ dz, double *__restrict__ dw,
                                                         double *__restrict__ aos,
                                                         ChunkExt *__restrict__ chunk_ext,
                                                         unsigned long long *__restrict__ xrange, int slab_later,
                                                         const RunRank rr) {
  // slab_later: the batch's slab entries and chunk extents are written in cell order by slab_append_run, for
  // which this kernel draws every node's (cell, rank in the cell) on the way (rr; one launch less per batch)
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long m = 0ull;
  unsigned long long xlo = ~0ull, xhi = 0ull, ylo = ~0ull, yhi = 0ull, zlo = ~0ull, zhi = 0ull;
  if (i < n) {
    const double a = pos[i * dim + 0], b = pos[i * dim + 1], c = pos[i * dim + 2];
    x[base + i] = a; y[base + i] = b; z[base + i] = c;
    const double sa = a - ox, sb = b - oy, sc = c - oz;
    const float fa = (float)sa, fb = (float)sb, fc = (float)sc;
    xf[base + i] = fa; yf[base + i] = fb; zf[base + i] = fc;
    // slab index: a new node sits at position == index until the next rebuild; its chunk's
    // x extent grows accordingly (a NaN x can never be within range of anything: not tracked)
    if (!slab_later) {
      sx[base + i] = fa; sy[base + i] = fb; sz[base + i] = fc;
      dx[base + i] = a; dy[base + i] = b; dz[base + i] = c;
      sid[base + i] = (int32_t)(base + i);
    }
    if (slab_later) {
      const int cell = cell_of(a, b, rr.sp->x0, rr.sp->inv_wx, rr.sp->Kx, rr.sp->y0, rr.sp->inv_wy, rr.sp->Ky);
      rr.sr[i] = make_int2(cell, atomicAdd(&rr.hist[cell], 1));
    }
    if (a == a) xlo = xhi = enc_ord(a);
    if (b == b) ylo = yhi = enc_ord(b);
    if (c == c) zlo = zhi = enc_ord(c);
    double pp = (double)fa * (double)fa + (double)fb * (double)fb + (double)fc * (double)fc;
    m = max(max((unsigned long long)__double_as_longlong(fabs(sa)), (unsigned long long)__double_as_longlong(fabs(sb))),
            (unsigned long long)__double_as_longlong(fabs(sc)));
    if (dim == 4) {
      const double d = pos[i * dim + 3];
      w[base + i] = d;
      const double sd = d - ow;
      const float fd = (float)sd;
      wf[base + i] = fd;
      if (!slab_later) { sw[base + i] = fd; dw[base + i] = d; }
      pp += (double)fd * (double)fd;
      m = max(m, (unsigned long long)__double_as_longlong(fabs(sd)));
    }
    ppf[base + i] = (float)pp;
    if (!slab_later) spp[base + i] = (float)pp;
    reinterpret_cast<double4 *>(aos)[base + i] = make_double4(a, b, c, dim == 4 ? pos[i * dim + 3] : 0.0);
  }
  // chunk extents: the 64 positions of a wave lie in one chunk unless they straddle a chunk
  // boundary; then one lane updates the chunk with the wave's extent, otherwise every lane its own
  const long long ch = (base + i) / kSlabChunk;
  const long long ch_first = (base + ((long long)blockIdx.x * blockDim.x + (threadIdx.x & ~63))) / kSlabChunk;
  const bool one_chunk = __ballot(i < n && ch != ch_first) == 0ull;
  if (!one_chunk && i < n && !slab_later) {
    if (xlo != ~0ull) { atomicMin(&chunk_ext[ch].xlo, xlo); atomicMax(&chunk_ext[ch].xhi, xhi); }
    if (ylo != ~0ull) { atomicMin(&chunk_ext[ch].ylo, ylo); atomicMax(&chunk_ext[ch].yhi, yhi); }
  }
  for (int off = 32; off > 0; off >>= 1) {
    unsigned long long o = __shfl_xor(m, off);
    m = max(m, o);
    o = __shfl_xor(xlo, off);
    xlo = min(xlo, o);
    o = __shfl_xor(xhi, off);
    xhi = max(xhi, o);
    o = __shfl_xor(ylo, off);
    ylo = min(ylo, o);
    o = __shfl_xor(yhi, off);
    yhi = max(yhi, o);
    o = __shfl_xor(zlo, off);
    zlo = min(zlo, o);
    o = __shfl_xor(zhi, off);
    zhi = max(zhi, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (one_chunk && !slab_later) {
      if (xlo != ~0ull) { atomicMin(&chunk_ext[ch_first].xlo, xlo); atomicMax(&chunk_ext[ch_first].xhi, xhi); }
      if (ylo != ~0ull) { atomicMin(&chunk_ext[ch_first].ylo, ylo); atomicMax(&chunk_ext[ch_first].yhi, yhi); }
    }
    // the bounds of the whole tree rarely move: look first (a stale look only costs an atomic that changes nothing)
    if (m != 0ull && m > *absmax) atomicMax(absmax, m);
    if (xlo != ~0ull) {
      if (xlo < xrange[0]) atomicMin(&xrange[0], xlo);
      if (xhi > xrange[1]) atomicMax(&xrange[1], xhi);
    }
    if (ylo != ~0ull) {
      if (ylo < xrange[2]) atomicMin(&xrange[2], ylo);
      if (yhi > xrange[3]) atomicMax(&xrange[3], yhi);
    }
    if (zlo != ~0ull) {
      if (zlo < xrange[4]) atomicMin(&xrange[4], zlo);
      if (zhi > xrange[5]) atomicMax(&xrange[5], zhi);
    }
  }
}

// room for n more edges in the mirror (the five arrays double from 4096, keeping what they hold); RRTX_E_CAPACITY
// beyond the int32 id range.  Waits on the stream when it has to reallocate.
int grow_edges(rrtx_ctx *ctx, int64_t n) {
  if (ctx->ge_n + n > 0x7fffffffll) return fail(ctx, RRTX_E_CAPACITY, "edge ids are int32");
  if (ctx->ge_n + n <= ctx->ge_cap) return RRTX_OK;
  int64_t nc = ctx->ge_cap > 0 ? ctx->ge_cap : 4096;
  while (nc < ctx->ge_n + n) nc *= 2;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int rc;
  if ((rc = regrow(ctx, ctx->ge_start, nc, ctx->ge_n))) return rc;
  if ((rc = regrow(ctx, ctx->ge_end, nc, ctx->ge_n))) return rc;
  if ((rc = regrow(ctx, ctx->ge_dist, nc, ctx->ge_n))) return rc;
  if ((rc = regrow(ctx, ctx->ge_dist0, nc, ctx->ge_n))) return rc;
  if ((rc = regrow(ctx, ctx->ge_dirty, nc, ctx->ge_n))) return rc;
  if ((rc = regrow(ctx, ctx->ge_culled, nc, ctx->ge_n))) return rc;
  RRTX_HIP(ctx, hipMemsetAsync(ctx->ge_culled + ctx->ge_n, 0, (size_t)(nc - ctx->ge_n), ctx->stream));   // no new edge is culled
  ctx->ge_cap = nc;
  return RRTX_OK;
}

int grow_nodes(rrtx_ctx *ctx, int64_t need) {
  if (need <= ctx->cap_nodes) return RRTX_OK;
  int64_t nc = ctx->cap_nodes > 0 ? ctx->cap_nodes : 1024;
  while (nc < need) nc *= 2;
  if (nc > 0x7fffffffll) return fail(ctx, RRTX_E_CAPACITY, "node index space is int32 (%lld requested)", (long long)need);
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  int rc;
  for (int k = 0; k < ctx->dim; ++k) {
    if ((rc = regrow(ctx, ctx->nodes[k], nc, ctx->n_nodes))) return rc;
    if ((rc = regrow(ctx, ctx->nodes_f[k], nc, ctx->n_nodes))) return rc;
    if ((rc = regrow(ctx, ctx->sl_f[k], nc, ctx->n_nodes))) return rc;
    if ((rc = regrow(ctx, ctx->sl_d[k], nc, ctx->n_nodes))) return rc;
  }
  if ((rc = regrow(ctx, ctx->nodes_pp, nc, ctx->n_nodes))) return rc;
  if ((rc = regrow(ctx, ctx->nodes_aos, 4 * nc, 4 * ctx->n_nodes))) return rc;   // (four doubles a node)
  if ((rc = regrow(ctx, ctx->sl_pp, nc, ctx->n_nodes))) return rc;
  if ((rc = regrow(ctx, ctx->sl_id, nc, ctx->n_nodes))) return rc;
  {
    // chunk extents: new chunks start empty (min = ~0, max = 0)
    const int64_t nch = nc / kSlabChunk + 1;
    const int64_t old = ctx->cap_chunks;
    if ((rc = regrow(ctx, ctx->chunk_ext, nch, old))) return rc;
    std::vector<ChunkExtHost> empty((size_t)(nch - old), ChunkExtHost{~0ull, 0ull, ~0ull, 0ull});
    RRTX_HIP(ctx, hipMemcpy(ctx->chunk_ext + old, empty.data(), sizeof(ChunkExtHost) * empty.size(), hipMemcpyHostToDevice));
    ctx->cap_chunks = nch;
  }
  if (!ctx->d_absmax.p) {
    RRTX_HIP(ctx, ctx->d_absmax.ensure(sizeof(unsigned long long)));
    RRTX_HIP(ctx, hipMemset(ctx->d_absmax.p, 0, sizeof(unsigned long long)));
    const unsigned long long none[6] = {~0ull, 0ull, ~0ull, 0ull, ~0ull, 0ull};
    RRTX_HIP(ctx, ctx->d_xrange.ensure(sizeof(none)));
    RRTX_HIP(ctx, hipMemcpy(ctx->d_xrange.p, none, sizeof(none), hipMemcpyHostToDevice));
  }
  ctx->cap_nodes = nc;
  return RRTX_OK;
}

// ---- host <-> device transfers of the host-pointer entry points ----
static bool host_registered(const rrtx_ctx *ctx, const void *p, size_t bytes) {
  const char *c = static_cast<const char *>(p);
  for (const auto &r : ctx->h_registered)
    if (c >= r.first && c + bytes <= r.first + r.second) return true;
  return false;
}
// room for `bytes` more in the pinned arena; a call reserves its whole need up front (arena_begin), so the arena never
// moves while copies into it are in flight
static int arena_begin(rrtx_ctx *ctx, size_t need) {
  ctx->h_arena_used = 0;
  ctx->h_pending.clear();
  if (need <= ctx->h_arena.bytes) return RRTX_OK;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  size_t nb = 1 << 20;
  while (nb < need) nb *= 2;
  RRTX_HIP(ctx, ctx->h_arena.alloc(nb, hipHostMallocDefault));   // (nothing of a finished call is kept)
  return RRTX_OK;
}
static char *arena_take(rrtx_ctx *ctx, size_t bytes) {
  const size_t at = (ctx->h_arena_used + 63) & ~(size_t)63;
  if (at + bytes > ctx->h_arena.bytes) return nullptr;
  ctx->h_arena_used = at + bytes;
  return ctx->h_arena.as<char>() + at;
}
// device -> caller array: straight DMA when the array is registered, else through the arena (copied out by
// arena_flush after the stream has been synchronised)
// Only SMALL results are staged (a 16 KB pageable destination costs a driver-side bounce of its own, ~35 us against
// ~20 us pinned): measured on the MI355X box (tools/pcie_probe.py), a pageable destination of a megabyte or more
// receives its DMA at the same ~50 GB/s as a pinned one, while a staged copy has to be read back from DRAM by one host
// thread at a third of that.  An output the caller did not ask for (null) or an empty one is skipped.
constexpr size_t kSmallIn = 1u << 20, kSmallOut = 256u << 10;
// what stage_in_small / d2h take from the arena for an array of that size (a call's reservation is the sum of these)
size_t small_in(size_t bytes) { return bytes <= kSmallIn ? bytes + 64 : 0; }
size_t small_out(size_t bytes) { return bytes <= kSmallOut ? bytes + 64 : 0; }
static int d2h(rrtx_ctx *ctx, void *dst, const void *src_dev, size_t bytes) {
  if (!dst || !bytes) return RRTX_OK;
  void *to = dst;
  if (bytes <= kSmallOut && !host_registered(ctx, dst, bytes)) {
    char *a = arena_take(ctx, bytes);
    if (a) { to = a; ctx->h_pending.push_back({dst, a, bytes}); }
  }
  RRTX_HIP(ctx, hipMemcpyAsync(to, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return RRTX_OK;
}
static void arena_flush(rrtx_ctx *ctx) {
  for (const auto &c : ctx->h_pending) std::memcpy(c.dst, c.src, c.bytes);
  ctx->h_pending.clear();
}

// stage a host array on the device workspace `buf`
hipError_t stage_in(rrtx_ctx *ctx, DevBuf &buf, const void *host, size_t bytes) {
  hipError_t e = buf.ensure(bytes ? bytes : 8);
  if (e == hipSuccess && bytes) e = hipMemcpyAsync(buf.p, host, bytes, hipMemcpyHostToDevice, ctx->stream);
  return e;
}
// two host arrays of the same size (the endpoints of a batch of edges) -> ws_q, ws_q2
hipError_t stage_pair(rrtx_ctx *ctx, const double *s, const double *g, size_t bytes) {
  hipError_t e = stage_in(ctx, ctx->ws_q, s, bytes);
  return e != hipSuccess ? e : stage_in(ctx, ctx->ws_q2, g, bytes);
}
// queue the copy of a device result straight into caller memory; an output the caller did not ask for (null) or an
// empty one is skipped.  The caller synchronises once all its copies are queued.
hipError_t copy_out(rrtx_ctx *ctx, void *dst, const void *src_dev, size_t bytes) {
  return dst && bytes ? hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream) : hipSuccess;
}
// the entry count of a two-call entry point, read back after whatever the caller has queued before it
hipError_t read_count(rrtx_ctx *ctx, const void *count_dev, int64_t *count) {
  hipError_t e = hipMemcpyAsync(count, count_dev, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream);
  return e != hipSuccess ? e : hipStreamSynchronize(ctx->stream);
}
// the capacity step of a two-call entry point: report the count, and refuse it above cap before any entry is copied
int check_capacity(rrtx_ctx *ctx, const char *fn, const char *noun, int64_t count, int64_t cap, int64_t *needed) {
  if (needed) *needed = count;
  if (count > cap) return fail(ctx, RRTX_E_CAPACITY, "%s: %lld %s, capacity %lld", fn, (long long)count, noun, (long long)cap);
  return RRTX_OK;
}
// samples with an empty ball (nearest index -1): resolve with the full nearest scan
int nearest_fallback(rrtx_ctx *ctx, const double *q, int nq, int dim, int32_t *nearest_idx, double *nearest_dist) {
  std::vector<int> miss;
  for (int i = 0; i < nq; ++i) if (nearest_idx[i] < 0) miss.push_back(i);
  if (miss.empty()) return RRTX_OK;
  std::vector<double> mq(miss.size() * (size_t)dim);
  for (size_t k = 0; k < miss.size(); ++k) std::memcpy(&mq[k * dim], q + (size_t)miss[k] * dim, sizeof(double) * dim);
  std::vector<int32_t> mi(miss.size());
  std::vector<double> md(miss.size());
  int rc = rrtx_nn_nearest(ctx, mq.data(), (int)miss.size(), mi.data(), md.data());
  if (rc) return rc;
  for (size_t k = 0; k < miss.size(); ++k) { nearest_idx[miss[k]] = mi[k]; nearest_dist[miss[k]] = md[k]; }
  return RRTX_OK;
}
// the samples of a batched call: through the pinned arena when they are small (one host memcpy of cache-resident data,
// then a pinned H2D), so the driver does not bounce them itself.  Call after arena_begin.
static int stage_in_small(rrtx_ctx *ctx, DevBuf &buf, const void *host, size_t bytes) {
  RRTX_HIP(ctx, buf.ensure(bytes ? bytes : 8));
  if (!bytes) return RRTX_OK;
  const void *from = host;
  if (bytes <= kSmallIn && !host_registered(ctx, host, bytes)) {
    char *a = arena_take(ctx, bytes);
    if (a) { std::memcpy(a, host, bytes); from = a; }
  }
  RRTX_HIP(ctx, hipMemcpyAsync(buf.p, from, bytes, hipMemcpyHostToDevice, ctx->stream));
  return RRTX_OK;
}

// ---- packed blocks: what a batched call holds per sample, in one allocation so that it moves in one transfer ----
// A block is described once, as an ordered list of typed fields (Field / take of block_layout.hpp; the structs below):
// that gives the byte size of the transfer and every field's address under any base, the device block or its pinned copy.
// (a block is made from its sample count alone, B{n}: the fields are then initialised in the order they are declared,
// which is the layout, and `bytes` grows with them to the size of the block)
struct CandidatesBlock {            // rrtx_extend_candidates[_dubins]; the _self calls: its CSR prefix alone
  size_t n, bytes = 0;
  Field<int64_t> offsets = take<int64_t>(bytes, n + 1), count = take<int64_t>(bytes, 1);
  size_t csr_bytes = bytes;
  Field<double> nearest_dist = take<double>(bytes, n);
  Field<int32_t> nearest_idx = take<int32_t>(bytes, n);
  Field<uint8_t> sample_unsafe = take<uint8_t>(bytes, n);
};
struct ClosestInBlock {             // rrtx_extend_closest_self[_dubins]: what goes up beside the samples
  size_t n, bytes = 0;
  Field<int32_t> tree_idx = take<int32_t>(bytes, n);
  Field<uint8_t> skip = take<uint8_t>(bytes, n), want = take<uint8_t>(bytes, n);
};
struct ClosestBlock {               // rrtx_extend_closest_self: per sample, the row length and the tree column
  size_t n, bytes = 0;
  Field<int32_t> count = take<int32_t>(bytes, n);
  Field<uint8_t> tree_hit_out = take<uint8_t>(bytes, n), tree_hit_in = take<uint8_t>(bytes, n);
};
constexpr size_t kWordBytes = 3;    // a Dubins word: three bytes an edge
struct ClosestDubinsBlock {         // rrtx_extend_closest_self_dubins: the same, the tree column with costs and words
  size_t n, bytes = 0;
  Field<double> tree_cost_out = take<double>(bytes, n), tree_cost_in = take<double>(bytes, n);
  Field<int32_t> count = take<int32_t>(bytes, n);
  Field<uint8_t> tree_word_out = take<uint8_t>(bytes, kWordBytes * n), tree_word_in = take<uint8_t>(bytes, kWordBytes * n);
  Field<uint8_t> tree_hit_out = take<uint8_t>(bytes, n), tree_hit_in = take<uint8_t>(bytes, n);
};
struct SelectBlock {                // rrtx_extend_select
  size_t n, bytes = 0;
  Field<int64_t> counts = take<int64_t>(bytes, 2);              // list entries, rewire entries
  Field<int64_t> rw_offsets = take<int64_t>(bytes, n + 1), parent_entry = take<int64_t>(bytes, n);
  Field<double> lmc_new = take<double>(bytes, n), nearest_dist = take<double>(bytes, n);
  Field<int32_t> parent_idx = take<int32_t>(bytes, n), nearest_idx = take<int32_t>(bytes, n);
  Field<uint8_t> status = take<uint8_t>(bytes, n), sample_unsafe = take<uint8_t>(bytes, n);
  Field<int64_t> offsets = take<int64_t>(bytes, n + 1, 8);      // the tail: leaves only if the caller wants the lists
  size_t bytes_without_lists = offsets.off;
};
struct TargetQueryBlock {           // find_new_target: the poses still searching, one block per round side
  size_t n, dim, bytes = 0;
  Field<double> pose = take<double>(bytes, n * dim), rad = take<double>(bytes, n);
  Field<double> thr = take<double>(bytes, 2 * n);               // thr_lt of every pose, then thr_gt
  Field<int32_t> slot = take<int32_t>(bytes, n);
};
struct TargetResultBlock {          // find_new_target: what leaves at the end, then the rounds' own words
  size_t n, bytes = 0;
  Field<double> cost_to_goal = take<double>(bytes, n), edge_dist = take<double>(bytes, n), radius_used = take<double>(bytes, n);
  Field<int32_t> target_idx = take<int32_t>(bytes, n), rounds = take<int32_t>(bytes, n);
  Field<uint8_t> status = take<uint8_t>(bytes, n);
  size_t result_bytes = bytes;
  Field<int32_t> pending = take<int32_t>(bytes, n, 8);
  Field<int64_t> hdr = take<int64_t>(bytes, 3, 8);              // TargetRound::hdr
};
// The first `bytes` of a device block on their way down into the pinned arena (queued; after arena_begin, which has
// reserved block_need(bytes) for it): *host = where the fields are read once the stream has been waited for.
size_t block_need(size_t bytes) { return bytes + 64; }
int block_down(rrtx_ctx *ctx, const char *fn, const void *dev, size_t bytes, char **host) {
  if (!(*host = arena_take(ctx, bytes))) return fail(ctx, RRTX_E_NOMEM, "%s: staging arena", fn);
  RRTX_HIP(ctx, hipMemcpyAsync(*host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return RRTX_OK;
}
// skip, want and tree_idx of a closest call (null: the field stays as it is) gathered in the arena and sent up to ws_q2
// in one transfer (after arena_begin, which has reserved block_need(I.bytes) for it)
int closest_inputs_up(rrtx_ctx *ctx, const char *fn, const ClosestInBlock &I, const uint8_t *skip, const uint8_t *want,
                      const int32_t *tree_idx) {
  RRTX_HIP(ctx, ctx->ws_q2.ensure(I.bytes));
  char *up = arena_take(ctx, I.bytes);
  if (!up) return fail(ctx, RRTX_E_NOMEM, "%s: staging arena", fn);
  I.tree_idx.from(tree_idx, up); I.skip.from(skip, up); I.want.from(want, up);
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_q2.p, up, I.bytes, hipMemcpyHostToDevice, ctx->stream));
  return RRTX_OK;
}

// thr_first_ge / thr_first_gt of per-query radii r[i * r_stride] (a run of equal radii is worked out once)
void fill_thresholds(const double *r, int r_stride, int nq, double *lt, double *gt) {
  double last_r = std::nan(""), l = 0, g = 0;
  for (int i = 0; i < nq; ++i) {
    const double ri = r[(size_t)i * r_stride];
    if (!(ri == last_r)) { last_r = ri; l = thr_first_ge(ri); g = thr_first_gt(ri); }
    lt[i] = l; gt[i] = g;
  }
}

// rrtLMC of a call: the caller's host array staged into ws_sel_lmc, or (null) the context's own array as
// rrtx_node_cost_set left it.  Call after arena_begin, which has reserved lmc_arena_need for it (what stage_in_small
// takes from the arena for an array of that size).
struct Lmc { const double *dev; int64_t n; };
size_t lmc_arena_need(const rrtx_ctx *ctx, const double *lmc_host) {
  return lmc_host ? small_in(sizeof(double) * (size_t)ctx->n_nodes) : 0;
}
int resolve_lmc(rrtx_ctx *ctx, const double *lmc_host, Lmc *lmc) {
  int rc = lmc_host ? stage_in_small(ctx, ctx->ws_sel_lmc, lmc_host, sizeof(double) * (size_t)ctx->n_nodes) : node_cost_ensure(ctx);
  *lmc = lmc_host ? Lmc{ctx->ws_sel_lmc.as<double>(), ctx->n_nodes} : Lmc{ctx->node_lmc, ctx->node_lmc_n};
  return rc;
}

// The neighbour lists of a call on the device, `cap` entries a column (the closest calls: nq * k slots).  Here and
// nowhere else is it written which workspace holds which column: idx in ws_out_idx, owner in ws_owner, the double
// columns one after the other in ws_out_dist, the flag bytes out / in in ws_out_u8a / _u8b with the words behind them.
// cols = 1: SimpleEdge's one cost column, which is key, cost_out and cost_in alike; cols = 3: the Dubins key | cost_out |
// cost_in.  words: the Dubins word columns (null without).  The addresses are taken after every ensure; lists that are
// held (sel_hold_*) are found again with the arguments they were made with, which then ensure nothing anew.  offsets and
// count are the call's own (null here): it sets them once the block that holds them is ensured.
int neighbour_lists(rrtx_ctx *ctx, int64_t cap, int cols, bool words, Lists *L) {
  const size_t n = (size_t)std::max<int64_t>(cap, 1);
  RRTX_HIP(ctx, ctx->ws_out_idx.ensure(sizeof(int32_t) * n));
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * n));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * (size_t)cols * n));
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure((words ? 1 + kWordBytes : 1) * n));
  RRTX_HIP(ctx, ctx->ws_out_u8b.ensure((words ? 1 + kWordBytes : 1) * n));
  double *key = ctx->ws_out_dist.as<double>();
  uint8_t *out = ctx->ws_out_u8a.as<uint8_t>(), *in = ctx->ws_out_u8b.as<uint8_t>();
  *L = Lists{nullptr, nullptr, ctx->ws_out_idx.as<int32_t>(), ctx->ws_owner.as<int32_t>(), key,
             EdgeCols{cols == 3 ? key + n : key, cols == 3 ? key + 2 * n : key, words ? out + n : nullptr,
                      words ? in + n : nullptr, out, in}, cap};
  return RRTX_OK;
}
// the caller's arrays for the columns of a call's lists (null: not asked for, or the call has no such column)
struct ListsOut { int32_t *idx; double *key, *cost_out, *cost_in; uint8_t *word_out, *word_in, *hit_out, *hit_in; };
// fn(caller's array, device column, bytes an entry) for every column
template <class Fn>
int each_column_out(const Lists &L, const ListsOut &to, Fn fn) {
  int rc = fn(to.key, L.key, sizeof(double));
  if (!rc) rc = fn(to.cost_out, L.e.cost_out, sizeof(double));
  if (!rc) rc = fn(to.cost_in, L.e.cost_in, sizeof(double));
  if (!rc) rc = fn(to.idx, L.idx, sizeof(int32_t));
  if (!rc) rc = fn(to.word_out, L.e.word_out, kWordBytes);
  if (!rc) rc = fn(to.word_in, L.e.word_in, kWordBytes);
  if (!rc) rc = fn(to.hit_out, L.e.hit_out, 1);
  return rc ? rc : fn(to.hit_in, L.e.hit_in, 1);
}
// the first n entries of the columns the caller asked for, queued (d2h skips a null array)
int lists_down(rrtx_ctx *ctx, const Lists &L, int64_t n, const ListsOut &to) {
  return each_column_out(L, to, [&](void *dst, const void *src, size_t entry) { return d2h(ctx, dst, src, entry * (size_t)n); });
}
// what d2h may take from the arena for up to `cap` entries of `entry` bytes, ...
size_t out_need(const void *dst, size_t entry, int64_t cap) {
  return !dst ? 0 : small_out((size_t)cap > kSmallOut / entry ? kSmallOut : entry * (size_t)cap);
}
// ... and for the lists of a call
size_t lists_need(const ListsOut &to, int64_t cap) {
  size_t need = 0;
  each_column_out(Lists{}, to, [&](const void *dst, const void *, size_t entry) { need += out_need(dst, entry, cap); return 0; });
  return need;
}
// the end of a call that queued n entries or slots: the transfers waited for, the staged ones copied to the caller
int lists_finish(rrtx_ctx *ctx, int64_t n) {
  if (n <= 0) return RRTX_OK;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  arena_flush(ctx);
  return RRTX_OK;
}

// The lists of rrtx_extend_select and find_new_target stay on the device.  Their capacity is the context's business:
// sized once from what the last search produced, and when an attempt produces more, grown to that with an eighth of
// headroom and the attempt made once more.  `attempt` enqueues the search and what follows it over lists of L.cap
// entries; the `bytes` at `dev`, which begin with the int64 count of entries the search produced, are then read back
// into the arena at `host`.  offsets: the CSR of the attempt (ensured by the caller), which with the count completes L.
template <class Attempt>
int with_neighbour_lists(rrtx_ctx *ctx, const char *fn, int nq, int64_t at_least, int cols, int64_t *offsets, void *host,
                         int64_t *dev, size_t bytes, Attempt attempt) {
  int64_t cap = ctx->sel_list_cap > 0 ? ctx->sel_list_cap
                                      : std::max<int64_t>(ctx->last_neighbors + ctx->last_neighbors / 8, std::max<int64_t>(64 * (int64_t)nq, 1024));
  cap = std::max(cap, at_least);
  for (int again = 0;; ++again) {
    Lists L;
    int rc = neighbour_lists(ctx, cap, cols, false, &L);
    if (rc) return rc;
    L.offsets = offsets; L.count = dev;
    ctx->sel_list_cap = cap;
    rc = attempt(L);
    if (rc) return rc;
    RRTX_HIP(ctx, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t total = *static_cast<const int64_t *>(host);
    ctx->last_neighbors = total;
    if (total <= cap) return RRTX_OK;
    if (again) return fail(ctx, RRTX_E_STATE, "%s: %lld neighbours after growing to %lld", fn, (long long)total, (long long)cap);
    cap = total + total / 8;
  }
}

std::string g_create_err;
std::mutex g_create_mu;

}  // namespace
}  // namespace rrtx

using namespace rrtx;

// The end of a context, also of one rrtx_create could not finish (no stream yet, or a node store grown in part): what is
// not memory is undone here; every allocation is then released by the member that owns it.
rrtx_ctx::~rrtx_ctx() {
  (void)hipSetDevice(device);
  if (stream) (void)hipStreamSynchronize(stream);
  drain_spans(this);
  for (auto ev : event_pool) (void)hipEventDestroy(ev);
  for (const auto &r : h_registered) (void)hipHostUnregister(const_cast<char *>(r.first));
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

#define CHECK_CTX_KEEP(ctx)            \
  ::rrtx::ApiRange _rrtx_api_range(__func__); \
  do {                                 \
    if (!(ctx)) return RRTX_E_INVALID; \
    hipError_t _sd = hipSetDevice((ctx)->device); \
    if (_sd != hipSuccess) return fail((ctx), RRTX_E_DEVICE, "hipSetDevice(%d): %s", (ctx)->device, hipGetErrorString(_sd)); \
  } while (0)
// The lists rrtx_extend_select[_dubins] leaves for rrtx_graph_edges_append_selected live in workspaces most entry points write
// (ws_out_idx / _dist / _u8a / _u8b, ws_sel_blk), so dropping the record of them is the rule and keeping it the
// exception: CHECK_CTX_KEEP is for the entry points that write none of those workspaces (include/rrtx.h lists them).
#define CHECK_CTX(ctx)  \
  CHECK_CTX_KEEP(ctx);  \
  (ctx)->sel_hold_nq = -1

extern "C" {

const char *rrtx_create_error(void) { return g_create_err.c_str(); }

int rrtx_sq_thresholds(double r, double *first_ge, double *first_gt) {
  if (!first_ge || !first_gt) return RRTX_E_INVALID;
  *first_ge = thr_first_ge(r);
  *first_gt = thr_first_gt(r);
  return RRTX_OK;
}

int rrtx_create(rrtx_ctx **out, int dim, int device, int64_t node_capacity) {
  std::lock_guard<std::mutex> lk(g_create_mu);
  if (!out) { g_create_err = "out is NULL"; return RRTX_E_INVALID; }
  *out = nullptr;
  if (dim != 3 && dim != 4) { g_create_err = "dim must be 3 or 4"; return RRTX_E_INVALID; }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_err = std::string("no HIP device available: ") + hipGetErrorString(e);
    return RRTX_E_DEVICE;
  }
  if (device < 0 || device >= ndev) { g_create_err = "device ordinal out of range"; return RRTX_E_INVALID; }
  e = hipSetDevice(device);
  if (e != hipSuccess) { g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e); return RRTX_E_DEVICE; }
  rrtx_ctx *ctx = new (std::nothrow) rrtx_ctx();
  if (!ctx) { g_create_err = "out of host memory"; return RRTX_E_NOMEM; }
  ctx->dim = dim;
  ctx->device = device;
  e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    g_create_err = std::string("hipStreamCreate: ") + hipGetErrorString(e);
    delete ctx;
    return RRTX_E_DEVICE;
  }
  ctx->stream = ctx->own_stream;
  int rc = grow_nodes(ctx, node_capacity > 0 ? node_capacity : 1024);
  if (rc != RRTX_OK) {
    g_create_err = ctx->err;
    delete ctx;
    return rc;
  }
  *out = ctx;
  return RRTX_OK;
}

int rrtx_destroy(rrtx_ctx *ctx) {
  if (!ctx) return RRTX_E_INVALID;
  delete ctx;
  return RRTX_OK;
}

const char *rrtx_last_error(rrtx_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int rrtx_set_stream(rrtx_ctx *ctx, void *hip_stream) {
  CHECK_CTX(ctx);
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;
  return RRTX_OK;
}

void *rrtx_get_stream(rrtx_ctx *ctx) { return ctx ? reinterpret_cast<void *>(ctx->stream) : nullptr; }

int rrtx_sync(rrtx_ctx *ctx) {
  CHECK_CTX_KEEP(ctx);
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_profile(rrtx_ctx *ctx, int enable) {
  CHECK_CTX(ctx);
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  drain_spans(ctx);
  for (int k = 0; k < KF_COUNT; ++k) { ctx->fam_ms[k] = 0.0; ctx->fam_launches[k] = 0; }
  ctx->profiling = enable < 0 ? 0 : (enable > 2 ? 2 : enable);
  return RRTX_OK;
}

int rrtx_set_option(rrtx_ctx *ctx, int option, int64_t value) {
  CHECK_CTX(ctx);
  switch (option) {
    case RRTX_OPT_NN_FILTER: ctx->opt_nn_filter = value != 0; return RRTX_OK;
    case RRTX_OPT_SCAN_BLOCKS: ctx->opt_scan_blocks = value > 0 ? (int)value : 1280; return RRTX_OK;
    case RRTX_OPT_SCAN_ITEMS: ctx->opt_scan_items = value > 0 ? (int)value : 2048; return RRTX_OK;
    case RRTX_OPT_SCAN_TILE_Q: ctx->opt_tile_q = value > 0 ? (int)value : 0; return RRTX_OK;
    case RRTX_OPT_NN_CULL: ctx->opt_nn_cull = value < 0 ? 0 : (value > 2 ? 2 : (int)value); return RRTX_OK;
    case RRTX_OPT_PROFILE_EVERY: ctx->opt_profile_every = value > 1 ? (int)value : 1; return RRTX_OK;
    case RRTX_OPT_KNN_LISTS: ctx->opt_knn_lists = value != 0; return RRTX_OK;
    case RRTX_OPT_EXTEND_OBSTACLES: ctx->opt_extend_polygons = value == 1; return RRTX_OK;
    case RRTX_OPT_TUNE: ctx->opt_tune = (int)value; return RRTX_OK;
    case RRTX_OPT_ROOT_RULE: ctx->opt_root_rule = value != 0; return RRTX_OK;
    case RRTX_OPT_SPACE_HAS_TIME:
      if (value != 0 && ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "a space with time is [x y t theta]: dim = 4");
      ctx->opt_space_has_time = value != 0;
      return RRTX_OK;
    case RRTX_OPT_DUBINS_TIME_COLUMN:
      if (value != RRTX_TIME_COLUMN_PIECEWISE && value != RRTX_TIME_COLUMN_RUNNING_SUM)
        return fail(ctx, RRTX_E_INVALID, "set_option: RRTX_OPT_DUBINS_TIME_COLUMN is 0 (piecewise) or 1 (running sum), not %lld",
                    (long long)value);
      ctx->opt_dubins_time_column = (int)value;
      return RRTX_OK;
    case RRTX_OPT_NEAREST_REC_CAP: ctx->opt_nearest_rec_cap = value > 0 ? (long long)value : 0; return RRTX_OK;
    case RRTX_OPT_BUCKET_MULT: {
      int m = 2;
      while (m < value && m < 16) m *= 2;
      ctx->bkt_mult = m;
      return RRTX_OK;
    }
    case RRTX_OPT_SELECT_LIST_CAP: ctx->sel_list_cap = value > 0 ? value : 0; return RRTX_OK;
    default: return fail(ctx, RRTX_E_INVALID, "set_option: unknown option %d", option);
  }
}

int rrtx_host_register(rrtx_ctx *ctx, void *ptr, size_t bytes) {
  CHECK_CTX(ctx);
  if (!ptr || bytes == 0) return fail(ctx, RRTX_E_INVALID, "host_register: bad arguments");
  if (host_registered(ctx, ptr, bytes)) return RRTX_OK;
  RRTX_HIP(ctx, hipHostRegister(ptr, bytes, hipHostRegisterDefault));
  ctx->h_registered.push_back({static_cast<const char *>(ptr), bytes});
  return RRTX_OK;
}

int rrtx_host_unregister(rrtx_ctx *ctx, void *ptr) {
  CHECK_CTX(ctx);
  for (size_t k = 0; k < ctx->h_registered.size(); ++k)
    if (ctx->h_registered[k].first == static_cast<const char *>(ptr)) {
      RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      RRTX_HIP(ctx, hipHostUnregister(ptr));
      ctx->h_registered.erase(ctx->h_registered.begin() + (long)k);
      return RRTX_OK;
    }
  return fail(ctx, RRTX_E_INVALID, "host_unregister: %p was not registered with this context", ptr);
}

int rrtx_get_option(rrtx_ctx *ctx, int option, int64_t *value) {
  CHECK_CTX_KEEP(ctx);
  if (!value) return fail(ctx, RRTX_E_INVALID, "get_option: null output");
  switch (option) {
    case RRTX_OPT_NN_FILTER: *value = ctx->opt_nn_filter ? 1 : 0; return RRTX_OK;
    case RRTX_OPT_SCAN_BLOCKS: *value = ctx->opt_scan_blocks; return RRTX_OK;
    case RRTX_OPT_SCAN_ITEMS: *value = ctx->opt_scan_items; return RRTX_OK;
    case RRTX_OPT_SCAN_TILE_Q: *value = ctx->opt_tile_q; return RRTX_OK;
    case RRTX_OPT_NN_CULL: *value = ctx->opt_nn_cull; return RRTX_OK;
    case RRTX_OPT_PROFILE_EVERY: *value = ctx->opt_profile_every; return RRTX_OK;
    case RRTX_OPT_KNN_LISTS: *value = ctx->opt_knn_lists ? 1 : 0; return RRTX_OK;
    case RRTX_OPT_EXTEND_OBSTACLES: *value = ctx->opt_extend_polygons ? 1 : 0; return RRTX_OK;
    case RRTX_OPT_TUNE: *value = ctx->opt_tune; return RRTX_OK;
    case RRTX_OPT_ROOT_RULE: *value = ctx->opt_root_rule ? 1 : 0; return RRTX_OK;
    case RRTX_OPT_SPACE_HAS_TIME: *value = ctx->opt_space_has_time ? 1 : 0; return RRTX_OK;
    case RRTX_OPT_DUBINS_TIME_COLUMN: *value = ctx->opt_dubins_time_column; return RRTX_OK;
    case RRTX_OPT_NEAREST_REC_CAP: *value = (int64_t)ctx->opt_nearest_rec_cap; return RRTX_OK;
    case RRTX_OPT_BUCKET_MULT: *value = ctx->bkt_mult; return RRTX_OK;
    case RRTX_OPT_LAST_PLACEMENT: *value = ctx->last_placement; return RRTX_OK;
    case RRTX_OPT_SELECT_LIST_CAP: *value = ctx->sel_list_cap; return RRTX_OK;
    default: return fail(ctx, RRTX_E_INVALID, "get_option: unknown option %d", option);
  }
}

int rrtx_last_tile_form(rrtx_ctx *ctx, int *form) {
  CHECK_CTX_KEEP(ctx);
  if (!form) return fail(ctx, RRTX_E_INVALID, "last_tile_form: null output");
  *form = ctx->last_tile_form;
  return RRTX_OK;
}

int rrtx_stats(rrtx_ctx *ctx, rrtx_stats_t *out) {
  CHECK_CTX_KEEP(ctx);
  if (!out) return fail(ctx, RRTX_E_INVALID, "stats: out is NULL");
  drain_spans(ctx);
  out->n_nodes = ctx->n_nodes;
  out->dim = ctx->dim;
  out->n_spheres = (int32_t)ctx->sph_active.size();
  out->n_polygons = (int32_t)ctx->poly_active.size();
  out->n_wraps = ctx->n_wraps;
  out->ms_nn_scan = ctx->fam_ms[KF_NN_SCAN];       out->launches_nn_scan = ctx->fam_launches[KF_NN_SCAN];
  out->ms_nn_finish = ctx->fam_ms[KF_NN_FINISH];   out->launches_nn_finish = ctx->fam_launches[KF_NN_FINISH];
  out->ms_nn_nearest = ctx->fam_ms[KF_NN_NEAREST]; out->launches_nn_nearest = ctx->fam_launches[KF_NN_NEAREST];
  out->ms_edges = ctx->fam_ms[KF_EDGES];           out->launches_edges = ctx->fam_launches[KF_EDGES];
  out->ms_points = ctx->fam_ms[KF_POINTS];         out->launches_points = ctx->fam_launches[KF_POINTS];
  out->ms_dubins = ctx->fam_ms[KF_DUBINS];         out->launches_dubins = ctx->fam_launches[KF_DUBINS];
  out->ms_dubins_steer = ctx->fam_ms[KF_DUBINS_STEER]; out->launches_dubins_steer = ctx->fam_launches[KF_DUBINS_STEER];
  out->last_sweep_candidates = ctx->last_sweep_candidates;
  out->last_pairs = ctx->last_pairs;
  out->last_neighbors = ctx->last_neighbors;
  out->last_tile_q = ctx->last_tile_q;
  out->last_scan_units = 0;
  if (ctx->last_culled) {
    int u = 0;
    int rc = scan_units(ctx, &u);
    if (rc) return rc;
    out->last_scan_units = u;
  }
  return RRTX_OK;
}

// ---- tree ---------------------------------------------------------------------------
int64_t rrtx_nodes_count(rrtx_ctx *ctx) { return ctx ? ctx->n_nodes : 0; }

static int nodes_append_args(rrtx_ctx *ctx, const double *pos, int64_t n) {
  if (n < 0 || (n > 0 && !pos)) return fail(ctx, RRTX_E_INVALID, "nodes_append: bad arguments");
  return RRTX_OK;
}

int rrtx_nodes_append_dev(rrtx_ctx *ctx, const double *pos_dev, int64_t n) {
  CHECK_CTX_KEEP(ctx);
  int rc = nodes_append_args(ctx, pos_dev, n);
  if (rc || n == 0) return rc;
  if ((rc = grow_nodes(ctx, ctx->n_nodes + n))) return rc;
  if (!ctx->origin_set) {
    // origin of the fp32 shadow = the first node (the tree root); one small read-back, once per ctx
    double first[4] = {0, 0, 0, 0};
    RRTX_HIP(ctx, hipMemcpyAsync(first, pos_dev, sizeof(double) * ctx->dim, hipMemcpyDeviceToHost, ctx->stream));
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < ctx->dim; ++k) ctx->origin[k] = std::isfinite(first[k]) ? first[k] : 0.0;
    ctx->origin_set = true;
  }
  const bool as_run = slab_run_wanted(ctx, n);
  RunRank rr;
  rr.sp = nullptr; rr.hist = nullptr; rr.sr = nullptr;
  if (as_run) {
    rc = slab_run_prepare(ctx, n, &rr);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(aos_to_soa_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, pos_dev,
                     ctx->dim, (long long)n, (long long)ctx->n_nodes, ctx->origin[0], ctx->origin[1], ctx->origin[2],
                     ctx->origin[3], ctx->nodes[0], ctx->nodes[1], ctx->nodes[2],
                     ctx->nodes[ctx->dim == 4 ? 3 : 2], ctx->nodes_f[0], ctx->nodes_f[1], ctx->nodes_f[2],
                     ctx->nodes_f[ctx->dim == 4 ? 3 : 2], ctx->nodes_pp, ctx->d_absmax.as<unsigned long long>(),
                     ctx->sl_f[0], ctx->sl_f[1], ctx->sl_f[2], ctx->sl_f[ctx->dim == 4 ? 3 : 2], ctx->sl_pp, ctx->sl_id,
                     ctx->sl_d[0], ctx->sl_d[1], ctx->sl_d[2], ctx->sl_d[ctx->dim == 4 ? 3 : 2], ctx->nodes_aos,
                     reinterpret_cast<ChunkExt *>(ctx->chunk_ext.get()), ctx->d_xrange.as<unsigned long long>(), as_run ? 1 : 0, rr);
  RRTX_HIP(ctx, hipGetLastError());
  if (as_run) {
    rc = slab_append_run(ctx, ctx->n_nodes, n);
    if (rc) return rc;
  }
  ctx->n_nodes += n;
  return RRTX_OK;
}

int rrtx_nodes_append(rrtx_ctx *ctx, const double *pos, int64_t n, int64_t *first_index) {
  CHECK_CTX_KEEP(ctx);
  int rc = nodes_append_args(ctx, pos, n);
  if (rc) return rc;
  if (first_index) *first_index = ctx->n_nodes;
  if (n == 0) return RRTX_OK;
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q, pos, sizeof(double) * (size_t)n * ctx->dim));
  rc = rrtx_nodes_append_dev(ctx, ctx->ws_q.as<double>(), n);
  if (rc) return rc;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_set_wrap(rrtx_ctx *ctx, int dim_index, double period) {
  CHECK_CTX(ctx);
  if (dim_index < 0 || dim_index >= ctx->dim || !(period > 0.0))
    return fail(ctx, RRTX_E_INVALID, "set_wrap: dimension %d / period %g invalid", dim_index, period);
  for (int w = 0; w < ctx->n_wraps; ++w)
    if (ctx->wrap_dim[w] == dim_index) { ctx->wrap_period[w] = period; return RRTX_OK; }
  if (ctx->n_wraps >= kMaxWraps) return fail(ctx, RRTX_E_CAPACITY, "at most %d wrapped dimensions", kMaxWraps);
  ctx->wrap_dim[ctx->n_wraps] = dim_index;
  ctx->wrap_period[ctx->n_wraps] = period;
  ctx->n_wraps += 1;
  return RRTX_OK;
}

// ---- obstacles -----------------------------------------------------------------------
int rrtx_spheres_set(rrtx_ctx *ctx, const double *cxyzr, const uint8_t *active, int m) {
  CHECK_CTX(ctx);
  if (m < 0 || (m > 0 && !cxyzr)) return fail(ctx, RRTX_E_INVALID, "spheres_set: bad arguments");
  ctx->sph.assign(cxyzr, cxyzr + 4 * (size_t)m);
  ctx->sph_active.assign((size_t)m, 1);
  if (active) for (int i = 0; i < m; ++i) ctx->sph_active[i] = active[i] ? 1 : 0;
  ctx->sph_dirty = true;
  return RRTX_OK;
}

int rrtx_obstacle_update(rrtx_ctx *ctx, int which, double radius, uint8_t active) {
  CHECK_CTX(ctx);
  if (which < 0 || which >= (int)ctx->sph_active.size())
    return fail(ctx, RRTX_E_INVALID, "obstacle_update: index %d out of range", which);
  ctx->sph[4 * (size_t)which + 3] = radius;
  ctx->sph_active[which] = active ? 1 : 0;
  ctx->sph_dirty = true;
  return RRTX_OK;
}

int rrtx_polygons_set(rrtx_ctx *ctx, const int32_t *vert_off, const double *vxy, const double *centre_radius,
                      const uint8_t *kind, const uint8_t *active, int m) {
  CHECK_CTX(ctx);
  if (m < 0 || (m > 0 && (!vert_off || !vxy))) return fail(ctx, RRTX_E_INVALID, "polygons_set: bad arguments");
  for (int i = 0; i < m; ++i)
    if (vert_off[i + 1] < vert_off[i]) return fail(ctx, RRTX_E_INVALID, "polygons_set: vert_off not monotone");
  ctx->poly_off.assign(vert_off, vert_off + (m > 0 ? m + 1 : 0));
  if (m == 0) ctx->poly_off.assign(1, 0);
  const int nv = m > 0 ? vert_off[m] : 0;
  ctx->poly_vxy.assign(vxy, vxy + 2 * (size_t)nv);
  ctx->poly_kind.assign((size_t)m, 3);
  ctx->poly_active.assign((size_t)m, 1);
  if (kind) for (int i = 0; i < m; ++i) ctx->poly_kind[i] = kind[i];
  if (active) for (int i = 0; i < m; ++i) ctx->poly_active[i] = active[i] ? 1 : 0;
  ctx->poly_cr.assign(3 * (size_t)m, 0.0);
  for (int i = 0; i < m; ++i) {
    const int kd = ctx->poly_kind[i];
    if (kd != 1 && kd != 3 && kd != 6 && kd != 7)
      return fail(ctx, RRTX_E_INVALID, "polygons_set: obstacle kind %d not supported (1, 3, 6 or 7)", kd);
    if (centre_radius) {
      for (int k = 0; k < 3; ++k) ctx->poly_cr[3 * (size_t)i + k] = centre_radius[3 * (size_t)i + k];
      continue;
    }
    // Obstacle(kind, polygon) ctor, R/DRRT_data_structures.jl:229-241: Julia's maximum / minimum, which keep a NaN
    // (a polygon with a NaN vertex has a NaN circle, which the bounding-circle tests never rule out)
    const int b = vert_off[i], e = vert_off[i + 1];
    if (e <= b) continue;
    double maxx = vxy[2 * b], minx = maxx, maxy = vxy[2 * b + 1], miny = maxy;
    for (int v = b + 1; v < e; ++v) {
      maxx = jl_max(maxx, vxy[2 * v]); minx = jl_min(minx, vxy[2 * v]);
      maxy = jl_max(maxy, vxy[2 * v + 1]); miny = jl_min(miny, vxy[2 * v + 1]);
    }
    const double px = (maxx + minx) / 2.0, py = (maxy + miny) / 2.0;
    double best = 0.0;
    for (int v = b; v < e; ++v) {
      double dx = vxy[2 * v] - px, dy = vxy[2 * v + 1] - py;
      double s = dx * dx + dy * dy;
      best = v == b ? s : jl_max(best, s);
    }
    ctx->poly_cr[3 * (size_t)i + 0] = px;
    ctx->poly_cr[3 * (size_t)i + 1] = py;
    ctx->poly_cr[3 * (size_t)i + 2] = std::sqrt(best);
  }
  ctx->poly_path_off.assign((size_t)m + 1, 0);
  ctx->poly_path.clear();
  ctx->poly_dirty = true;
  return RRTX_OK;
}

int rrtx_polygon_paths_set(rrtx_ctx *ctx, const int32_t *path_off, const double *path_xyt, int m) {
  CHECK_CTX(ctx);
  if (m != (int)ctx->poly_kind.size())
    return fail(ctx, RRTX_E_INVALID, "polygon_paths_set: %d paths for %d polygons", m, (int)ctx->poly_kind.size());
  if (m > 0 && !path_off) return fail(ctx, RRTX_E_INVALID, "polygon_paths_set: bad arguments");
  if (m == 0) return RRTX_OK;
  if (path_off[0] != 0) return fail(ctx, RRTX_E_INVALID, "polygon_paths_set: path_off must start at 0");
  for (int i = 0; i < m; ++i)
    if (path_off[i + 1] < path_off[i]) return fail(ctx, RRTX_E_INVALID, "polygon_paths_set: path_off not monotone");
  if (path_off[m] > 0 && !path_xyt) return fail(ctx, RRTX_E_INVALID, "polygon_paths_set: bad arguments");
  ctx->poly_path_off.assign(path_off, path_off + m + 1);
  ctx->poly_path.assign(path_xyt, path_xyt + 3 * (size_t)path_off[m]);
  ctx->poly_dirty = true;
  return RRTX_OK;
}

// obstacle.obstacleUnused of k list positions (R/DRRT.jl:3287 and the discovery of an obstacle): the flags alone, the
// shapes and paths stay; the device tables are packed again at the next sync, as after rrtx_polygons_set
int rrtx_polygons_set_active(rrtx_ctx *ctx, const int32_t *obstacles, int k, const uint8_t *active) {
  CHECK_CTX(ctx);
  const int m = (int)ctx->poly_active.size();
  if (k < 0 || (k > 0 && (!obstacles || !active))) return fail(ctx, RRTX_E_INVALID, "polygons_set_active: bad arguments");
  for (int j = 0; j < k; ++j)
    if (obstacles[j] < 0 || obstacles[j] >= m)
      return fail(ctx, RRTX_E_INVALID, "polygons_set_active: obstacle %d (entry %d) out of range (%d polygons)", obstacles[j], j, m);
  if (k == 0) return RRTX_OK;
  for (int j = 0; j < k; ++j) ctx->poly_active[(size_t)obstacles[j]] = active[j] ? 1 : 0;
  ctx->poly_dirty = true;
  return RRTX_OK;
}

// ---- nearest neighbours ----------------------------------------------------------------
// (argument checks shared by each host-pointer entry point and its _dev twin)
static int nn_nearest_args(rrtx_ctx *ctx, const double *q, int nq, const int32_t *idx, const double *dist) {
  if (nq < 0 || (nq > 0 && (!q || !idx || !dist))) return fail(ctx, RRTX_E_INVALID, "nn_nearest: bad arguments");
  return RRTX_OK;
}

int rrtx_nn_nearest_dev(rrtx_ctx *ctx, const double *q, int nq, int32_t *idx, double *dist) {
  CHECK_CTX(ctx);
  int rc = nn_nearest_args(ctx, q, nq, idx, dist);
  return rc ? rc : launch_nn_nearest(ctx, q, nq, idx, dist);
}

int rrtx_nn_nearest(rrtx_ctx *ctx, const double *q, int nq, int32_t *idx, double *dist) {
  CHECK_CTX(ctx);
  int rc = nn_nearest_args(ctx, q, nq, idx, dist);
  if (rc || nq == 0) return rc;
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q, q, sizeof(double) * (size_t)nq * ctx->dim));
  RRTX_HIP(ctx, ctx->ws_out_idx.ensure(sizeof(int32_t) * (size_t)nq));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * (size_t)nq));
  rc = launch_nn_nearest(ctx, ctx->ws_q.as<double>(), nq, ctx->ws_out_idx.as<int32_t>(), ctx->ws_out_dist.as<double>());
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, idx, ctx->ws_out_idx.p, sizeof(int32_t) * (size_t)nq));
  RRTX_HIP(ctx, copy_out(ctx, dist, ctx->ws_out_dist.p, sizeof(double) * (size_t)nq));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

static int nn_knearest_args(rrtx_ctx *ctx, const double *q, int nq, const int32_t *idx, const double *dist,
                            const int32_t *count) {
  if (nq < 0 || (nq > 0 && (!q || !idx || !dist || !count)))
    return fail(ctx, RRTX_E_INVALID, "nn_knearest: bad arguments");
  return RRTX_OK;
}

int rrtx_nn_knearest_dev(rrtx_ctx *ctx, const double *q, int nq, int k, int32_t *idx, double *dist, int32_t *count) {
  CHECK_CTX(ctx);
  int rc = nn_knearest_args(ctx, q, nq, idx, dist, count);
  return rc ? rc : launch_nn_knearest(ctx, q, nq, k, idx, dist, count);
}

int rrtx_nn_knearest(rrtx_ctx *ctx, const double *q, int nq, int k, int32_t *idx, double *dist, int32_t *count) {
  CHECK_CTX(ctx);
  int rc = nn_knearest_args(ctx, q, nq, idx, dist, count);
  if (rc || nq == 0) return rc;
  const size_t stride = (size_t)(k < 2 ? 2 : k);
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q, q, sizeof(double) * (size_t)nq * ctx->dim));
  RRTX_HIP(ctx, ctx->ws_out_idx.ensure(sizeof(int32_t) * ((size_t)nq * stride + (size_t)nq)));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * (size_t)nq * stride));
  int32_t *idx_dev = ctx->ws_out_idx.as<int32_t>();
  int32_t *count_dev = idx_dev + (size_t)nq * stride;
  rc = launch_nn_knearest(ctx, ctx->ws_q.as<double>(), nq, k, idx_dev, ctx->ws_out_dist.as<double>(), count_dev);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, idx, idx_dev, sizeof(int32_t) * (size_t)nq * stride));
  RRTX_HIP(ctx, copy_out(ctx, dist, ctx->ws_out_dist.p, sizeof(double) * (size_t)nq * stride));
  RRTX_HIP(ctx, copy_out(ctx, count, count_dev, sizeof(int32_t) * (size_t)nq));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// (the _dev form takes one radius: r points at it, r_stride = 0)
static int nn_radius_args(rrtx_ctx *ctx, const double *q, const double *r, int r_stride, int nq, const int64_t *offsets,
                          const int32_t *idx, const double *dist, int64_t cap) {
  if (nq < 0 || cap < 0 || (nq > 0 && (!q || !r || !offsets)) || (cap > 0 && (!idx || !dist)) ||
      (r_stride != 0 && r_stride != 1))
    return fail(ctx, RRTX_E_INVALID, "nn_radius: bad arguments");
  return RRTX_OK;
}

int rrtx_nn_radius_dev(rrtx_ctx *ctx, const double *q, double r, int nq, int64_t *offsets, int32_t *idx,
                       double *dist, int64_t cap, int64_t *needed_dev) {
  CHECK_CTX(ctx);
  int rc = nn_radius_args(ctx, q, &r, 0, nq, offsets, idx, dist, cap);
  return rc ? rc : launch_nn_radius(ctx, q, nullptr, r, nq, offsets, idx, dist, cap, needed_dev);
}

int rrtx_nn_radius(rrtx_ctx *ctx, const double *q, const double *r, int r_stride, int nq, int64_t *offsets,
                   int32_t *idx, double *dist, int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  int rc = nn_radius_args(ctx, q, r, r_stride, nq, offsets, idx, dist, cap);
  if (rc) return rc;
  if (nq == 0) { if (needed) *needed = 0; if (offsets) offsets[0] = 0; return RRTX_OK; }
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q, q, sizeof(double) * (size_t)nq * ctx->dim));
  const double *thr_dev = nullptr;
  if (r_stride == 1) {
    std::vector<double> thr(2 * (size_t)nq);
    fill_thresholds(r, 1, nq, thr.data(), thr.data() + nq);
    RRTX_HIP(ctx, stage_in(ctx, ctx->ws_thr, thr.data(), sizeof(double) * thr.size()));
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));  // thr goes out of scope
    thr_dev = ctx->ws_thr.as<double>();
  }
  const int64_t dcap = cap > 0 ? cap : 1;
  RRTX_HIP(ctx, ctx->ws_out_off.ensure(sizeof(int64_t) * ((size_t)nq + 2)));
  RRTX_HIP(ctx, ctx->ws_out_idx.ensure(sizeof(int32_t) * (size_t)dcap));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * (size_t)dcap));
  int64_t *off_dev = ctx->ws_out_off.as<int64_t>();
  int64_t *needed_dev = off_dev + nq + 1;
  rc = launch_nn_radius(ctx, ctx->ws_q.as<double>(), thr_dev, r[0], nq, off_dev, ctx->ws_out_idx.as<int32_t>(),
                        ctx->ws_out_dist.as<double>(), cap, needed_dev);
  if (rc) return rc;
  int64_t total = 0;
  RRTX_HIP(ctx, copy_out(ctx, offsets, off_dev, sizeof(int64_t) * ((size_t)nq + 1)));
  RRTX_HIP(ctx, read_count(ctx, needed_dev, &total));
  ctx->last_neighbors = total;
  if ((rc = check_capacity(ctx, "nn_radius", "neighbours", total, cap, needed))) return rc;
  if (total > 0) {
    RRTX_HIP(ctx, copy_out(ctx, idx, ctx->ws_out_idx.p, sizeof(int32_t) * (size_t)total));
    RRTX_HIP(ctx, copy_out(ctx, dist, ctx->ws_out_dist.p, sizeof(double) * (size_t)total));
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return RRTX_OK;
}

// ---- collision ----------------------------------------------------------------------------
static int edges_check_args(rrtx_ctx *ctx, int kind, const double *p0, const double *p1, int64_t ne, const uint8_t *hit) {
  if (ne < 0 || (ne > 0 && (!p0 || !p1 || !hit)) || (kind != 0 && kind != 1))
    return fail(ctx, RRTX_E_INVALID, "edges_check: bad arguments");
  return RRTX_OK;
}

int rrtx_edges_check_dev(rrtx_ctx *ctx, int kind, const double *p0, const double *p1, int64_t ne,
                         double robot_radius, int obstacle_or_minus1, int obs_begin, int obs_end, uint8_t *hit,
                         int32_t *first_hit) {
  CHECK_CTX(ctx);
  int rc = edges_check_args(ctx, kind, p0, p1, ne, hit);
  if (rc) return rc;
  if (kind == 0)
    return launch_edges_spheres(ctx, p0, p1, ne, robot_radius, obstacle_or_minus1, obs_begin, obs_end, hit, first_hit);
  return launch_edges_polygons(ctx, p0, p1, ne, robot_radius, obstacle_or_minus1, obs_begin, obs_end, hit, first_hit);
}

int rrtx_edges_check(rrtx_ctx *ctx, int kind, const double *p0, const double *p1, int64_t ne, double robot_radius,
                     int obstacle_or_minus1, uint8_t *hit, int32_t *first_hit) {
  CHECK_CTX(ctx);
  int rc = edges_check_args(ctx, kind, p0, p1, ne, hit);
  if (rc || ne == 0) return rc;
  RRTX_HIP(ctx, stage_pair(ctx, p0, p1, sizeof(double) * (size_t)ne * ctx->dim));
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure((size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)ne));
  rc = rrtx_edges_check_dev(ctx, kind, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, robot_radius,
                            obstacle_or_minus1, -1, -1, ctx->ws_out_u8a.as<uint8_t>(),
                            first_hit ? ctx->ws_out_i32.as<int32_t>() : nullptr);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, hit, ctx->ws_out_u8a.p, (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, first_hit, ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_edges_check_idx(rrtx_ctx *ctx, const int32_t *start_idx, const int32_t *end_idx, int64_t ne,
                         double robot_radius, int obstacle_or_minus1, const uint8_t *obstacle_mask, uint8_t *hit,
                         int32_t *first_hit) {
  CHECK_CTX(ctx);
  if (ne < 0 || (ne > 0 && (!start_idx || !end_idx || !hit)))
    return fail(ctx, RRTX_E_INVALID, "edges_check_idx: bad arguments");
  if (ne == 0) return RRTX_OK;
  for (int64_t i = 0; i < ne; ++i)
    if (start_idx[i] < 0 || start_idx[i] >= ctx->n_nodes || end_idx[i] < 0 || end_idx[i] >= ctx->n_nodes)
      return fail(ctx, RRTX_E_INVALID, "edges_check_idx: edge %lld references a node outside [0, %lld)",
                  (long long)i, (long long)ctx->n_nodes);
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_i32a, start_idx, sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_i32b, end_idx, sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure((size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)ne));
  int rc = launch_edges_spheres(ctx, nullptr, nullptr, ne, robot_radius, obstacle_or_minus1, -1, -1,
                                ctx->ws_out_u8a.as<uint8_t>(), first_hit ? ctx->ws_out_i32.as<int32_t>() : nullptr,
                                ctx->ws_i32a.as<int32_t>(), ctx->ws_i32b.as<int32_t>(), obstacle_mask);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, hit, ctx->ws_out_u8a.p, (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, first_hit, ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// ---- obstacle sweeps over a device mirror of the planner's edges -----------------------
int64_t rrtx_graph_edges_count(rrtx_ctx *ctx) { return ctx ? ctx->ge_n : 0; }

int rrtx_graph_edges_clear(rrtx_ctx *ctx) {
  CHECK_CTX_KEEP(ctx);
  if (ctx->ge_n > 0) RRTX_HIP(ctx, hipMemsetAsync(ctx->ge_culled, 0, (size_t)ctx->ge_n, ctx->stream));
  ctx->ge_n = 0;
  graph_cost_forget(ctx);
  graph_delta_forget(ctx);
  return RRTX_OK;
}

int rrtx_graph_edges_append(rrtx_ctx *ctx, const int32_t *start_idx, const int32_t *end_idx, int64_t n,
                            int64_t *first_id) {
  CHECK_CTX_KEEP(ctx);
  if (n < 0 || (n > 0 && (!start_idx || !end_idx))) return fail(ctx, RRTX_E_INVALID, "graph_edges_append: bad arguments");
  if (first_id) *first_id = ctx->ge_n;
  if (n == 0) return RRTX_OK;
  for (int64_t i = 0; i < n; ++i)
    if (start_idx[i] < 0 || start_idx[i] >= ctx->n_nodes || end_idx[i] < 0 || end_idx[i] >= ctx->n_nodes)
      return fail(ctx, RRTX_E_INVALID, "graph_edges_append: edge %lld references a node outside [0, %lld)",
                  (long long)i, (long long)ctx->n_nodes);
  int rc = grow_edges(ctx, n);
  if (rc) return rc;
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ge_start + ctx->ge_n, start_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ge_end + ctx->ge_n, end_idx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  // edge.dist defaults to the SimpleEdge cost of the edge (rrtx_graph_edges_set_dist overrides it)
  int rc2 = launch_graph_edge_dist(ctx, ctx->ge_n, n);
  if (rc2) return rc2;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->ge_n += n;
  return RRTX_OK;
}

int rrtx_graph_edges_set_dist(rrtx_ctx *ctx, int64_t first_id, const double *dist, int64_t n) {
  CHECK_CTX_KEEP(ctx);
  if (n < 0 || first_id < 0 || first_id + n > ctx->ge_n || (n > 0 && !dist))
    return fail(ctx, RRTX_E_INVALID, "graph_edges_set_dist: edges [%lld, %lld) of %lld", (long long)first_id,
                (long long)(first_id + n), (long long)ctx->ge_n);
  if (n == 0) return RRTX_OK;
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ge_dist + first_id, dist, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  int rc = launch_graph_touch(ctx, first_id, n);
  if (rc) return rc;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

static int graph_edges_block_host(rrtx_ctx *ctx, const char *fn, bool restore, const int32_t *edge_ids, int64_t n) {
  if (n < 0 || (n > 0 && !edge_ids)) return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  for (int64_t i = 0; i < n; ++i)
    if (edge_ids[i] < 0 || edge_ids[i] >= ctx->ge_n) return fail(ctx, RRTX_E_INVALID, "%s: edge id %d out of range", fn, edge_ids[i]);
  return launch_graph_block(ctx, restore, edge_ids, n);
}

int rrtx_graph_edges_block(rrtx_ctx *ctx, const int32_t *edge_ids, int64_t n) {
  CHECK_CTX_KEEP(ctx);
  return graph_edges_block_host(ctx, "graph_edges_block", false, edge_ids, n);
}

int rrtx_graph_edges_unblock(rrtx_ctx *ctx, const int32_t *edge_ids, int64_t n) {
  CHECK_CTX_KEEP(ctx);
  return graph_edges_block_host(ctx, "graph_edges_unblock", true, edge_ids, n);
}

// ---- cullCurrentNeighbors over the mirror, and its compaction (kernels_cull.hip) --------------------------------
int rrtx_graph_edges_cull(rrtx_ctx *ctx, double ball, const int32_t *nodes, int64_t k, int64_t *n_culled) {
  CHECK_CTX_KEEP(ctx);
  if (n_culled) *n_culled = 0;
  if (!(ball >= 0.0)) return fail(ctx, RRTX_E_INVALID, "graph_edges_cull: the ball is negative or NaN");
  if (k < 0 || (k > 0 && !nodes)) return fail(ctx, RRTX_E_INVALID, "graph_edges_cull: bad arguments");
  for (int64_t i = 0; nodes && i < k; ++i)
    if (nodes[i] < 0 || nodes[i] >= ctx->n_nodes)
      return fail(ctx, RRTX_E_INVALID, "graph_edges_cull: node %d outside [0, %lld)", nodes[i], (long long)ctx->n_nodes);
  if (ctx->ge_n == 0 || (nodes && k == 0)) return RRTX_OK;
  return launch_edges_cull(ctx, ball, nodes, k, n_culled);
}

int rrtx_graph_edges_compact(rrtx_ctx *ctx, int32_t *remap, int64_t remap_cap, int64_t *n_removed) {
  CHECK_CTX_KEEP(ctx);
  if (n_removed) *n_removed = 0;
  if (remap && remap_cap < ctx->ge_n)
    return fail(ctx, RRTX_E_CAPACITY, "graph_edges_compact: remap has room for %lld of %lld edge ids", (long long)remap_cap,
                (long long)ctx->ge_n);
  if (ctx->ge_n == 0) return RRTX_OK;
  return launch_edges_compact(ctx, remap, n_removed);
}

int rrtx_graph_edges_get_culled(rrtx_ctx *ctx, int64_t first_id, int64_t n, uint8_t *culled) {
  CHECK_CTX_KEEP(ctx);
  if (n < 0 || first_id < 0 || first_id > ctx->ge_n || n > ctx->ge_n - first_id || (n > 0 && !culled))
    return fail(ctx, RRTX_E_INVALID, "graph_edges_get_culled: edges [%lld, %lld) of %lld", (long long)first_id,
                (long long)(first_id + n), (long long)ctx->ge_n);
  if (n == 0) return RRTX_OK;
  RRTX_HIP(ctx, copy_out(ctx, culled, ctx->ge_culled + first_id, (size_t)n));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// ---- neighbour lists -> mirror edges on the device (kernels_link.hip) -------------------------------------------
namespace {
int append_lists_args(rrtx_ctx *ctx, const char *fn, int nq, const int64_t *offsets, const int32_t *idx, const double *cost_out,
                      const double *cost_in, const uint8_t *hit_out, const uint8_t *hit_in, int64_t cap, const int32_t *node_of) {
  if (nq < 0 || cap < 0 || (nq > 0 && (!offsets || !node_of)) || (cap > 0 && (!idx || !cost_out || !cost_in || !hit_out || !hit_in)))
    return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  return RRTX_OK;
}

// The body the three entry points share, over lists on the device: the counting pass and the scan, ONE wait on the
// stream to read {entries, edges, verdict}, then the refusal or the growth of the mirror and the fill (enqueued).
// L.row_first null: the context's own array.
int append_lists_dev(rrtx_ctx *ctx, const char *fn, LinkLists L, int64_t *first_id, int64_t *n_added) {
  if (first_id) *first_id = ctx->ge_n;
  if (n_added) *n_added = 0;
  if (L.nq == 0) {
    if (L.row_first) RRTX_HIP(ctx, hipMemsetAsync(L.row_first, 0, sizeof(int64_t), ctx->stream));
    return RRTX_OK;
  }
  if (!L.row_first) {
    RRTX_HIP(ctx, ctx->ws_link_row.ensure(sizeof(int64_t) * ((size_t)L.nq + 1)));
    L.row_first = ctx->ws_link_row.as<int64_t>();
  }
  int rc = launch_link_count(ctx, L);
  if (rc) return rc;
  int64_t res[3] = {0, 0, 0};
  RRTX_HIP(ctx, hipMemcpyAsync(res, ctx->ws_link_res.p, sizeof(res), hipMemcpyDeviceToHost, ctx->stream));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const unsigned verdict = (unsigned)res[2];
  if (verdict & kLinkOverflow)
    return fail(ctx, RRTX_E_CAPACITY, "%s: the extend call produced more entries than the lists hold (%lld)", fn, (long long)L.lists.cap);
  if (verdict & kLinkBadOffsets) return fail(ctx, RRTX_E_INVALID, "%s: offsets out of order or beyond the lists", fn);
  if (verdict & kLinkBadNode)
    return fail(ctx, RRTX_E_INVALID, "%s: node_of references a node outside [0, %lld)", fn, (long long)ctx->n_nodes);
  if (verdict & kLinkBadIndex)
    return fail(ctx, RRTX_E_INVALID, "%s: a list entry references a %s", fn,
                L.idx_is_batch ? "batch position outside [0, nq)" : "node outside the tree");
  if (verdict & kLinkTooMany) return fail(ctx, RRTX_E_CAPACITY, "%s: edge ids are int32", fn);
  const int64_t total = res[1];
  if (total <= 0) return RRTX_OK;
  if ((rc = grow_edges(ctx, total))) return rc;
  if ((rc = launch_link_fill(ctx, L, ctx->ge_n, total))) return rc;
  ctx->ge_n += total;
  if (n_added) *n_added = total;
  return RRTX_OK;
}
}  // namespace

int rrtx_graph_edges_append_lists_dev(rrtx_ctx *ctx, int nq, const int64_t *offsets, const int32_t *idx,
                                      const double *cost_out, const double *cost_in, const uint8_t *hit_out,
                                      const uint8_t *hit_in, const int64_t *n_valid_dev, int64_t cap, const int32_t *node_of,
                                      int idx_is_batch, int64_t *first_id, int64_t *n_added, int64_t *row_first) {
  CHECK_CTX_KEEP(ctx);
  int rc = append_lists_args(ctx, "graph_edges_append_lists_dev", nq, offsets, idx, cost_out, cost_in, hit_out, hit_in, cap, node_of);
  if (rc) return rc;
  const ListsRO L{offsets, n_valid_dev, idx, nullptr, nullptr, {cost_out, cost_in, nullptr, nullptr, hit_out, hit_in}, cap};
  return append_lists_dev(ctx, "graph_edges_append_lists_dev", LinkLists{nq, L, node_of, idx_is_batch != 0, row_first}, first_id,
                          n_added);
}

int rrtx_graph_edges_append_lists(rrtx_ctx *ctx, int nq, const int64_t *offsets, const int32_t *idx, const double *cost_out,
                                  const double *cost_in, const uint8_t *hit_out, const uint8_t *hit_in, int64_t n_valid,
                                  int64_t cap, const int32_t *node_of, int idx_is_batch, int64_t *first_id, int64_t *n_added,
                                  int64_t *row_first) {
  CHECK_CTX(ctx);
  const char *fn = "graph_edges_append_lists";
  int rc = append_lists_args(ctx, fn, nq, offsets, idx, cost_out, cost_in, hit_out, hit_in, cap, node_of);
  if (rc) return rc;
  if (n_valid < 0) return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  if (first_id) *first_id = ctx->ge_n;
  if (n_added) *n_added = 0;
  if (n_valid > cap) return fail(ctx, RRTX_E_CAPACITY, "%s: %lld entries, capacity %lld", fn, (long long)n_valid, (long long)cap);
  if (nq == 0) { if (row_first) row_first[0] = 0; return RRTX_OK; }
  // the lists go up through the staging path of the host-pointer searches, into their workspaces; only the n_valid
  // entries the extend call produced travel, and they are the capacity the kernels check against
  const size_t n = (size_t)n_valid, rows = (size_t)nq + 1;
  const bool one_cost = cost_in == cost_out;
  rc = arena_begin(ctx, small_in(sizeof(int64_t) * rows) + small_in(sizeof(int32_t) * (size_t)nq) + small_in(sizeof(int32_t) * n) +
                            2 * small_in(sizeof(double) * n) + 2 * small_in(n) + small_out(sizeof(int64_t) * rows) + 512);
  if (rc) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_out_off, offsets, sizeof(int64_t) * rows))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_link_node, node_of, sizeof(int32_t) * (size_t)nq))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_out_idx, idx, sizeof(int32_t) * n))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_out_dist, cost_out, sizeof(double) * n))) return rc;
  if (!one_cost && (rc = stage_in_small(ctx, ctx->ws_out_f64, cost_in, sizeof(double) * n))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_out_u8a, hit_out, n))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_out_u8b, hit_in, n))) return rc;
  RRTX_HIP(ctx, ctx->ws_link_row.ensure(sizeof(int64_t) * rows));
  const double *co = ctx->ws_out_dist.as<double>();
  rc = append_lists_dev(ctx, fn,
                        LinkLists{nq, ListsRO{ctx->ws_out_off.as<int64_t>(), nullptr, ctx->ws_out_idx.as<int32_t>(), nullptr, nullptr,
                                              {co, one_cost ? co : ctx->ws_out_f64.as<double>(), nullptr, nullptr,
                                               ctx->ws_out_u8a.as<uint8_t>(), ctx->ws_out_u8b.as<uint8_t>()}, n_valid},
                                  ctx->ws_link_node.as<int32_t>(), idx_is_batch != 0, ctx->ws_link_row.as<int64_t>()},
                        first_id, n_added);
  if (rc) return rc;
  if (row_first && (rc = d2h(ctx, row_first, ctx->ws_link_row.p, sizeof(int64_t) * rows))) return rc;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  arena_flush(ctx);
  return RRTX_OK;
}

int rrtx_graph_edges_append_selected(rrtx_ctx *ctx, int nq, const int32_t *node_of, int64_t *first_id, int64_t *n_added,
                                     int64_t *row_first) {
  CHECK_CTX_KEEP(ctx);
  const char *fn = "graph_edges_append_selected";
  if (nq < 0 || (nq > 0 && !node_of)) return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  if (ctx->sel_hold_nq < 0)
    return fail(ctx, RRTX_E_STATE, "%s: the context holds no lists of rrtx_extend_select (none made, or a later call used "
                                   "their workspaces)", fn);
  if (ctx->sel_hold_nq != nq)
    return fail(ctx, RRTX_E_STATE, "%s: the held lists are those of %d samples, not %d", fn, ctx->sel_hold_nq, nq);
  if (first_id) *first_id = ctx->ge_n;
  if (n_added) *n_added = 0;
  if (nq == 0) { if (row_first) row_first[0] = 0; return RRTX_OK; }
  const size_t rows = (size_t)nq + 1;
  int rc = arena_begin(ctx, small_in(sizeof(int32_t) * (size_t)nq) + small_out(sizeof(int64_t) * rows) + 512);
  if (rc) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_link_node, node_of, sizeof(int32_t) * (size_t)nq))) return rc;
  RRTX_HIP(ctx, ctx->ws_link_row.ensure(sizeof(int64_t) * rows));
  const SelectBlock B{(size_t)nq};
  char *blk = ctx->ws_sel_blk.as<char>();
  Lists L;               // the held lists, as the select call made them
  if ((rc = neighbour_lists(ctx, ctx->sel_list_cap, ctx->sel_hold_cols, false, &L))) return rc;
  L.offsets = B.offsets.in(blk); L.count = B.counts.in(blk);
  rc = append_lists_dev(ctx, fn, LinkLists{nq, read_only(L), ctx->ws_link_node.as<int32_t>(), false, ctx->ws_link_row.as<int64_t>()},
                        first_id, n_added);
  if (rc) return rc;
  if (row_first && (rc = d2h(ctx, row_first, ctx->ws_link_row.p, sizeof(int64_t) * rows))) return rc;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));      // node_of is the caller's
  arena_flush(ctx);
  return RRTX_OK;
}

int rrtx_graph_edges_get(rrtx_ctx *ctx, const int32_t *ids, int64_t first_id, int64_t n, int32_t *start, int32_t *end,
                         double *dist, double *dist_original) {
  CHECK_CTX_KEEP(ctx);
  if (n < 0) return fail(ctx, RRTX_E_INVALID, "graph_edges_get: bad arguments");
  if (n == 0) return RRTX_OK;
  const size_t m = (size_t)n;
  if (!ids) {
    if (first_id < 0 || first_id > ctx->ge_n || n > ctx->ge_n - first_id)
      return fail(ctx, RRTX_E_INVALID, "graph_edges_get: edges [%lld, %lld) of %lld", (long long)first_id,
                  (long long)(first_id + n), (long long)ctx->ge_n);
    RRTX_HIP(ctx, copy_out(ctx, start, ctx->ge_start + first_id, sizeof(int32_t) * m));
    RRTX_HIP(ctx, copy_out(ctx, end, ctx->ge_end + first_id, sizeof(int32_t) * m));
    RRTX_HIP(ctx, copy_out(ctx, dist, ctx->ge_dist + first_id, sizeof(double) * m));
    RRTX_HIP(ctx, copy_out(ctx, dist_original, ctx->ge_dist0 + first_id, sizeof(double) * m));
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RRTX_OK;
  }
  for (int64_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= ctx->ge_n) return fail(ctx, RRTX_E_INVALID, "graph_edges_get: edge id %d out of range", ids[i]);
  RRTX_HIP(ctx, ctx->gc.ids.ensure(sizeof(int32_t) * m));
  RRTX_HIP(ctx, ctx->ws_link_get.ensure((2 * sizeof(double) + 2 * sizeof(int32_t)) * m));
  double *d_dist = ctx->ws_link_get.as<double>(), *d_dist0 = d_dist + m;
  int32_t *d_start = reinterpret_cast<int32_t *>(d_dist0 + m), *d_end = d_start + m;
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->gc.ids.p, ids, sizeof(int32_t) * m, hipMemcpyHostToDevice, ctx->stream));
  int rc = launch_link_gather(ctx, ctx->gc.ids.as<int32_t>(), n, start ? d_start : nullptr, end ? d_end : nullptr,
                              dist ? d_dist : nullptr, dist_original ? d_dist0 : nullptr);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, start, d_start, sizeof(int32_t) * m));
  RRTX_HIP(ctx, copy_out(ctx, end, d_end, sizeof(int32_t) * m));
  RRTX_HIP(ctx, copy_out(ctx, dist, d_dist, sizeof(double) * m));
  RRTX_HIP(ctx, copy_out(ctx, dist_original, d_dist0, sizeof(double) * m));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

namespace {
int graph_cost_args(rrtx_ctx *ctx, const char *fn, int root_idx, const double *lmc) {
  if (!lmc) return fail(ctx, RRTX_E_INVALID, "%s: lmc is NULL", fn);
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "%s on an empty tree", fn);
  if (root_idx < 0 || root_idx >= ctx->n_nodes) return fail(ctx, RRTX_E_INVALID, "%s: root %d out of range", fn, root_idx);
  return RRTX_OK;
}

int graph_cost_host(rrtx_ctx *ctx, const char *fn, int root_idx, bool update, double *lmc, int32_t *parent_edge, int32_t *passes) {
  int rc = graph_cost_args(ctx, fn, root_idx, lmc);
  if (rc) return rc;
  const size_t n = (size_t)ctx->n_nodes;
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * n));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * n));
  int np = 0;
  rc = launch_graph_cost(ctx, root_idx, update, ctx->ws_out_f64.as<double>(), parent_edge ? ctx->ws_out_i32.as<int32_t>() : nullptr, &np);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, lmc, ctx->ws_out_f64.p, sizeof(double) * n));
  RRTX_HIP(ctx, copy_out(ctx, parent_edge, ctx->ws_out_i32.p, sizeof(int32_t) * n));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (passes) *passes = np;
  return RRTX_OK;
}

int graph_cost_dev(rrtx_ctx *ctx, const char *fn, int root_idx, bool update, double *lmc_dev, int32_t *parent_edge_dev) {
  int rc = graph_cost_args(ctx, fn, root_idx, lmc_dev);
  return rc ? rc : launch_graph_cost(ctx, root_idx, update, lmc_dev, parent_edge_dev, nullptr);
}
}  // namespace

int rrtx_graph_cost_to_root(rrtx_ctx *ctx, int root_idx, double *lmc, int32_t *parent_edge, int32_t *passes) {
  CHECK_CTX_KEEP(ctx);
  return graph_cost_host(ctx, "graph_cost_to_root", root_idx, false, lmc, parent_edge, passes);
}

int rrtx_graph_cost_update(rrtx_ctx *ctx, int root_idx, double *lmc, int32_t *parent_edge, int32_t *passes) {
  CHECK_CTX_KEEP(ctx);
  return graph_cost_host(ctx, "graph_cost_update", root_idx, true, lmc, parent_edge, passes);
}

int rrtx_graph_cost_to_root_dev(rrtx_ctx *ctx, int root_idx, double *lmc_dev, int32_t *parent_edge_dev) {
  CHECK_CTX_KEEP(ctx);
  return graph_cost_dev(ctx, "graph_cost_to_root", root_idx, false, lmc_dev, parent_edge_dev);
}

int rrtx_graph_cost_update_dev(rrtx_ctx *ctx, int root_idx, double *lmc_dev, int32_t *parent_edge_dev) {
  CHECK_CTX_KEEP(ctx);
  return graph_cost_dev(ctx, "graph_cost_update", root_idx, true, lmc_dev, parent_edge_dev);
}

int rrtx_graph_cost_update_delta(rrtx_ctx *ctx, int root_idx, int store, int32_t *node, double *lmc, int32_t *parent_edge,
                                 int64_t cap, int64_t *needed, int32_t *passes) {
  CHECK_CTX_KEEP(ctx);
  if (cap < 0 || (cap > 0 && (!node || !lmc)) || !needed)
    return fail(ctx, RRTX_E_INVALID, "graph_cost_update_delta: bad arguments");
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "graph_cost_update_delta on an empty tree");
  if (root_idx < 0 || root_idx >= ctx->n_nodes)
    return fail(ctx, RRTX_E_INVALID, "graph_cost_update_delta: root %d out of range", root_idx);
  *needed = 0;
  const size_t dcap = cap > 0 ? (size_t)cap : 1;
  RRTX_HIP(ctx, ctx->ws_delta_node.ensure(sizeof(int32_t) * dcap));
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * dcap));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * dcap));
  int rc = arena_begin(ctx, 16 * (size_t)std::min<int64_t>(cap, ctx->n_nodes) + 256);
  if (rc) return rc;
  int np = 0;
  int64_t *total_dev = nullptr;
  rc = launch_graph_delta(ctx, root_idx, store != 0, ctx->ws_delta_node.as<int32_t>(), ctx->ws_out_f64.as<double>(),
                          ctx->ws_out_i32.as<int32_t>(), (long long)cap, &total_dev, &np);
  if (rc) return rc;
  if (passes) *passes = np;
  int64_t total = 0;
  RRTX_HIP(ctx, read_count(ctx, total_dev, &total));      // the call's one synchronisation before the records leave
  if ((rc = check_capacity(ctx, "graph_cost_update_delta", "changed nodes", total, cap, needed))) return rc;
  // the records fit: they go to the caller, and the baseline moves to the solver's state
  if ((rc = d2h(ctx, node, ctx->ws_delta_node.p, sizeof(int32_t) * (size_t)total))) return rc;
  if ((rc = d2h(ctx, lmc, ctx->ws_out_f64.p, sizeof(double) * (size_t)total))) return rc;
  if (parent_edge && (rc = d2h(ctx, parent_edge, ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)total))) return rc;
  if ((rc = launch_graph_delta_advance(ctx, root_idx))) return rc;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  arena_flush(ctx);
  return RRTX_OK;
}

// ---- obstacle sweeps of the polygon / Dubins space (R/DRRT.jl:3048-3290) ----------------------------------------
namespace {
// one query of findPointsInConflictWithObstacle: the point itself (the root is taken with <=) and its ghosts in the
// wrapped dimensions, in getNextGhostPoint's order and under its skip rule (R/ghostPoint.jl:60-111)
void push_query_with_ghosts(rrtx_ctx *ctx, const double q[4], double range, std::vector<SweepQuery> &out) {
  const double tlt = rrtx::thr_first_ge(range), tgt = rrtx::thr_first_gt(range);
  SweepQuery o = {q[0], q[1], q[2], q[3], tlt, ctx->opt_root_rule ? tgt : tlt};
  out.push_back(o);
  const int nw = ctx->n_wraps;
  for (int k = 1; k < (1 << nw); ++k) {
    double g[4] = {q[0], q[1], q[2], q[3]}, c[4] = {q[0], q[1], q[2], q[3]};
    for (int w = 0; w < nw; ++w) {
      if (!((k >> (nw - 1 - w)) & 1)) continue;
      const int d = ctx->wrap_dim[w];
      double dim_val = q[d], dim_closest = 0.0;
      if (q[d] < ctx->wrap_period[w] / 2.0) { dim_val += ctx->wrap_period[w]; dim_closest += ctx->wrap_period[w]; }
      else dim_val -= ctx->wrap_period[w];
      g[d] = dim_val; c[d] = dim_closest;
    }
    double s = 0.0;                          // KDdist(closestUnwrappedPoint, ghost)^2, left fold over the d coordinates
    for (int d = 0; d < ctx->dim; ++d) { const double t = c[d] - g[d]; s = (d == 0) ? t * t : s + t * t; }
    if (s >= tgt) continue;                  // > bestDist: this ghost is not searched (:104)
    SweepQuery gq = {g[0], g[1], g[2], g[3], tlt, tlt};
    out.push_back(gq);
  }
}

// the tail of a sweep entry point: read the count, refuse it above cap, queue the copy of the ids.  The caller
// synchronises (only when *total > 0: nothing is queued otherwise).
int sweep_ids_out(rrtx_ctx *ctx, const char *fn, const char *noun, const long long *total_dev, int32_t *edge_ids, int64_t cap,
                  int64_t *needed, int64_t *total) {
  RRTX_HIP(ctx, read_count(ctx, total_dev, total));
  const int rc = check_capacity(ctx, fn, noun, *total, cap, needed);
  if (rc) return rc;
  if (*total > 0) RRTX_HIP(ctx, copy_out(ctx, edge_ids, ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)*total));
  return RRTX_OK;
}

// sphere c = (x, y, z, radius) as a sweep's kernels read it: the SphRec of the edge test, the two thresholds of the range
SweepObs sweep_obs(const double *c, double robot_radius, double range, bool active) {
  SweepObs o;
  o.ob.cx = c[0]; o.ob.cy = c[1]; o.ob.cz = c[2];
  o.ob.thr = thr_first_gt(robot_radius + c[3]);
  o.thr_lt = thr_first_ge(range);
  o.thr_gt = thr_first_gt(range);
  o.active = active ? 1 : 0;
  o.pad0 = 0; o.pad1 = 0.0;
  return o;
}
}  // namespace

namespace {
// findPointsInConflictWithObstacle(S, KD, ob) for list position `obstacle` (R/DRRT.jl:3048-3125) as range queries,
// appended to qs: the static query, or one per path segment (kinds 6 / 7), each with its ghosts.  The obstacle's
// `active` flag is not read.  RRTX_E_STATE for what the reference refuses or has not coded.
int polygon_sweep_queries(rrtx_ctx *ctx, int obstacle, double robot_radius, double delta, std::vector<SweepQuery> &qs) {
  const bool dubins = ctx->dim == 4, has_time = ctx->opt_space_has_time;
  const int kind = ctx->poly_kind[obstacle];
  const double cx = ctx->poly_cr[3 * (size_t)obstacle], cy = ctx->poly_cr[3 * (size_t)obstacle + 1],
               rad = ctx->poly_cr[3 * (size_t)obstacle + 2];
  if (kind >= 1 && kind <= 5) {
    if (has_time) return fail(ctx, RRTX_E_STATE, "this type of obstacle not coded for this type of space (a static obstacle in a "
                              "space with time, R/DRRT.jl:3067)");
    // Euclidean space: range robotRadius + delta + radius around ob.position (a dim = 3 tree is the legacy 2-D space
    // embedded at z = 0); Dubins space: [x y 0.0 pi], range + pi
    const double q[4] = {cx, cy, 0.0, dubins ? 3.141592653589793 : 0.0};
    double range = robot_radius + delta + rad;
    if (dubins) range = range + 3.141592653589793;
    push_query_with_ghosts(ctx, q, range, qs);
  } else if (kind == 6 || kind == 7) {
    const int p0 = ctx->poly_path_off[obstacle], np = ctx->poly_path_off[obstacle + 1] - p0;
    if (np < 1) return fail(ctx, RRTX_E_STATE, "moving obstacle %d has no path (rrtx_polygon_paths_set)", obstacle);
    const double base = robot_radius + delta + rad;
    for (int i = 0; i < np; ++i) {
      const int j = (np == 1) ? 0 : i + 1;
      const double *pi = &ctx->poly_path[3 * (size_t)(p0 + i)], *pj = &ctx->poly_path[3 * (size_t)(p0 + j)];
      const double q[4] = {cx + (pi[0] + pj[0]) / 2.0, cy + (pi[1] + pj[1]) / 2.0, 0.0 + (pi[2] + pj[2]) / 2.0,
                           dubins ? 3.141592653589793 : 0.0};
      const double dx = pi[0] - pj[0], dy = pi[1] - pj[1], dt = pi[2] - pj[2];
      double range = base + std::sqrt((dx * dx + dy * dy) + dt * dt) / 2.0;
      if (dubins) range += 3.141592653589793;
      push_query_with_ghosts(ctx, q, range, qs);
      if (j == np - 1) break;
    }
  } else {
    return fail(ctx, RRTX_E_STATE, "this case not coded yet (obstacle kind %d, R/DRRT.jl:3121)", kind);
  }
  return RRTX_OK;
}
}  // namespace

int rrtx_obstacle_sweep_polygon(rrtx_ctx *ctx, int obstacle, double robot_radius, double delta, double r_min, int mode,
                                int32_t *edge_ids, int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  const int m = (int)ctx->poly_active.size();
  if (obstacle < 0 || obstacle >= m) return fail(ctx, RRTX_E_INVALID, "obstacle_sweep_polygon: obstacle %d out of range (%d polygons)", obstacle, m);
  if (cap < 0 || (cap > 0 && !edge_ids) || (mode != 0 && mode != 1)) return fail(ctx, RRTX_E_INVALID, "obstacle_sweep_polygon: bad arguments");
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "obstacle_sweep_polygon on an empty tree");
  const bool dubins = ctx->dim == 4;
  // ---- findPointsInConflictWithObstacle (R/DRRT.jl:3048-3125) ----
  std::vector<SweepQuery> qs;
  int rc = polygon_sweep_queries(ctx, obstacle, robot_radius, delta, qs);
  if (rc) return rc;
  if (needed) *needed = 0;
  ctx->last_sweep_candidates = 0;
  const long long ne = ctx->ge_n;
  if (ne == 0) return RRTX_OK;
  if ((rc = sync_polygons(ctx))) return rc;
  // the obstacle in the packed (in-use only) table: an unused obstacle collides with nothing (R/DRRT.jl:1525)
  const std::vector<int32_t> pos = active_positions(ctx->poly_active);
  int pb, pe;
  packed_range(pos, obstacle, obstacle + 1, pb, pe);
  if (pe <= pb) return RRTX_OK;
  rc = launch_sweep_mark_multi(ctx, qs.data(), (int)qs.size());
  if (rc) return rc;
  // ---- the out-edges (and parent edges) of those nodes; removeObstacle looks at blocked ones only ----
  RRTX_HIP(ctx, ctx->ws_i32a.ensure(sizeof(int32_t) * (size_t)ne));
  long long *total_dev = nullptr;
  int64_t n_c = 0;
  span_begin(ctx, KF_EDGES);
  rc = launch_sweep_select(ctx, mode == 1 ? 1 : 0, ctx->ws_i32a.as<int32_t>(), ne, &total_dev);
  span_end(ctx);
  if (rc) return rc;
  RRTX_HIP(ctx, read_count(ctx, total_dev, &n_c));
  ctx->last_sweep_candidates = n_c;
  if (n_c == 0) return RRTX_OK;
  // ---- explicitEdgeCheck(S, edge, ob) of every candidate; removeObstacle: and against every OTHER obstacle in use ----
  const int n_pass = mode == 1 ? 3 : 1;
  RRTX_HIP(ctx, ctx->ws_out_u8b.ensure((size_t)n_c * 3));
  uint8_t *hit = ctx->ws_out_u8b.as<uint8_t>(), *o1 = hit + n_c, *o2 = o1 + n_c;
  const int32_t *cand = ctx->ws_i32a.as<int32_t>();
  const int na = (int)pos.size();
  const int rb[3] = {pb, 0, pe}, re[3] = {pe, pb, na};       // ob | the packed obstacles before it | after it
  if (dubins) {
    for (int k = 0; k < n_pass; ++k) {
      rc = launch_dubins_edges_idx(ctx, cand, n_c, r_min, robot_radius, rb[k], re[k], hit + (size_t)k * n_c);
      if (rc) return rc;
    }
  } else {
    RRTX_HIP(ctx, ctx->ws_q.ensure(sizeof(double) * 3 * (size_t)n_c));
    RRTX_HIP(ctx, ctx->ws_q2.ensure(sizeof(double) * 3 * (size_t)n_c));
    rc = launch_sweep_gather(ctx, cand, n_c, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>());
    if (rc) return rc;
    const int lb[3] = {obstacle, 0, obstacle + 1}, le[3] = {obstacle + 1, obstacle, m};   // the same three ranges in list positions
    for (int k = 0; k < n_pass; ++k) {
      rc = launch_edges_polygons(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), n_c, robot_radius, -1, lb[k], le[k],
                                 hit + (size_t)k * n_c, nullptr);
      if (rc) return rc;
    }
  }
  const int64_t dcap = cap > 0 ? cap : 1;
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)dcap));
  span_begin(ctx, KF_EDGES);
  rc = launch_sweep_finish(ctx, cand, n_c, hit, mode == 1 ? o1 : nullptr, mode == 1 ? o2 : nullptr,
                           ctx->ws_out_i32.as<int32_t>(), cap, &total_dev);
  span_end(ctx);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = sweep_ids_out(ctx, "obstacle_sweep_polygon", "edges", total_dev, edge_ids, cap, needed, &total))) return rc;
  if (total > 0) RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// rrtx_obstacle_sweep_polygon_batch (release = false; apply: block the rows): mode 0 of rrtx_obstacle_sweep_polygon for a
// burst of list positions, CSR rows.  rrtx_obstacle_release_polygon_batch (release = true; apply: unblock them): the
// edge loops of a burst of removeObstacle calls (R/DRRT.jl:3202-3290), the members of the burst taken as gone together.
static int polygon_burst_host(rrtx_ctx *ctx, const char *fn, bool release, const int32_t *obstacles, int k, double robot_radius,
                              double delta, double r_min, int apply, int64_t *offsets, int32_t *edge_ids, int64_t cap,
                              int64_t *needed) {
  const int m = (int)ctx->poly_active.size();
  if (k < 0 || k > 65536 || !offsets || (k > 0 && !obstacles) || cap < 0 || (cap > 0 && !edge_ids))
    return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  for (int j = 0; j < k; ++j)
    if (obstacles[j] < 0 || obstacles[j] >= m)
      return fail(ctx, RRTX_E_INVALID, "%s: obstacle %d (entry %d) out of range (%d polygons)", fn, obstacles[j], j, m);
  if (needed) *needed = 0;
  if (k == 0) { offsets[0] = 0; return RRTX_OK; }
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "%s on an empty tree", fn);
  // every entry's queries first, in order: the first obstacle the single call would refuse fails the whole call before
  // anything runs.  Group g = entries [64 g, 64 g + 64), bit b of its words = entry 64 g + b.
  const int ng = (k + 63) / 64;
  std::vector<SweepQuery> qs;
  std::vector<int> qn((size_t)k);
  int rc;
  for (int j = 0; j < k; ++j) {
    const size_t before = qs.size();
    if ((rc = polygon_sweep_queries(ctx, obstacles[j], robot_radius, delta, qs))) return rc;
    qn[(size_t)j] = (int)(qs.size() - before);
  }
  if ((rc = sync_polygons(ctx))) return rc;
  // (the single call meets this only once it has a candidate to check; here it is asked before anything runs)
  if (ctx->dim == 4 && (rc = dubins_check_space(ctx))) return rc;
  ctx->last_sweep_candidates = 0;
  if (ctx->ge_n == 0) { std::fill(offsets, offsets + k + 1, (int64_t)0); return RRTX_OK; }
  // an obstacle that is not in use collides with nothing (R/DRRT.jl:1525): its queries stay out of the table
  const std::vector<int32_t> pos = active_positions(ctx->poly_active);
  std::vector<int32_t> packed((size_t)m, -1);
  for (size_t a = 0; a < pos.size(); ++a) packed[(size_t)pos[a]] = (int32_t)a;
  ctx->pswb_q_host.clear();
  ctx->pswb_qoff_host.assign((size_t)ng + 1, 0);
  ctx->pswb_pos_host.resize((size_t)k);
  size_t at = 0;
  for (int j = 0; j < k; ++j) {
    const int32_t p = packed[(size_t)obstacles[j]];
    ctx->pswb_pos_host[(size_t)j] = p;
    if (p >= 0)
      for (int i = 0; i < qn[(size_t)j]; ++i) ctx->pswb_q_host.push_back(SweepQueryOwned{qs[at + (size_t)i], 1ull << (j & 63), 0.0});
    at += (size_t)qn[(size_t)j];
    if ((j & 63) == 63 || j == k - 1) ctx->pswb_qoff_host[(size_t)(j >> 6) + 1] = (int)ctx->pswb_q_host.size();
  }
  ctx->prel_stay_host.clear();
  if (release) {
    // the obstacles that stay: the packed table less the in-use entries of the call, as the ranges between them -- the
    // single call's {0 .. pb}, {pe .. na} for one obstacle.  Empty ranges are dropped.
    std::vector<int32_t> gone;
    for (int j = 0; j < k; ++j)
      if (ctx->pswb_pos_host[(size_t)j] >= 0) gone.push_back(ctx->pswb_pos_host[(size_t)j]);
    std::sort(gone.begin(), gone.end());
    gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
    int32_t from = 0;
    for (const int32_t p : gone) {
      if (p > from) { ctx->prel_stay_host.push_back(from); ctx->prel_stay_host.push_back(p); }
      from = p + 1;
    }
    if ((int32_t)pos.size() > from) { ctx->prel_stay_host.push_back(from); ctx->prel_stay_host.push_back((int32_t)pos.size()); }
  }
  const int64_t dcap = cap > 0 ? cap : 1;
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)dcap));
  long long *total_dev = nullptr;
  if ((rc = launch_polygon_burst(ctx, k, r_min, robot_radius, release, ctx->ws_out_i32.as<int32_t>(), cap, &total_dev))) return rc;
  RRTX_HIP(ctx, copy_out(ctx, offsets, ctx->ws_swb_off.p, sizeof(int64_t) * (size_t)(k + 1)));
  int64_t total = 0;
  if ((rc = sweep_ids_out(ctx, fn, release ? "freed edges" : "colliding edges", total_dev, edge_ids, cap, needed, &total))) return rc;
  if (total > 0) {
    // addNewObstacle's dist = Inf / removeObstacle's dist = distOriginal for every id of every row, where the rows are
    if (apply && (rc = launch_graph_block_dev(ctx, release, ctx->ws_out_i32.as<int32_t>(), total))) return rc;
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return RRTX_OK;
}

int rrtx_obstacle_sweep_polygon_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, double robot_radius, double delta,
                                      double r_min, int block, int64_t *offsets, int32_t *edge_ids, int64_t cap,
                                      int64_t *needed) {
  CHECK_CTX(ctx);
  return polygon_burst_host(ctx, "obstacle_sweep_polygon_batch", false, obstacles, k, robot_radius, delta, r_min, block, offsets,
                            edge_ids, cap, needed);
}

int rrtx_obstacle_release_polygon_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, double robot_radius, double delta,
                                        double r_min, int unblock, int64_t *offsets, int32_t *edge_ids, int64_t cap,
                                        int64_t *needed) {
  CHECK_CTX(ctx);
  return polygon_burst_host(ctx, "obstacle_release_polygon_batch", true, obstacles, k, robot_radius, delta, r_min, unblock, offsets,
                            edge_ids, cap, needed);
}

int rrtx_dubins_edges_check_obstacle(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                                     double robot_radius, int obstacle, uint8_t *hit) {
  CHECK_CTX(ctx);
  const int m = (int)ctx->poly_active.size();
  if (ne < 0 || (ne > 0 && (!s || !g || !hit))) return fail(ctx, RRTX_E_INVALID, "dubins_edges_check_obstacle: bad arguments");
  if (obstacle < 0 || obstacle >= m) return fail(ctx, RRTX_E_INVALID, "dubins_edges_check_obstacle: obstacle %d out of range (%d polygons)", obstacle, m);
  if (ne == 0) return RRTX_OK;
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "Dubins steering needs a dim=4 [x y t theta] context");
  int pb, pe;
  packed_range(active_positions(ctx->poly_active), obstacle, obstacle + 1, pb, pe);
  if (pe <= pb) { std::memset(hit, 0, (size_t)ne); return RRTX_OK; }          // not in use: collides with nothing
  RRTX_HIP(ctx, stage_pair(ctx, s, g, sizeof(double) * (size_t)ne * 4));
  RRTX_HIP(ctx, ctx->ws_out_u8b.ensure((size_t)ne));
  int rc = launch_dubins_edges_check(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, r_min, robot_radius, nullptr,
                                     nullptr, ctx->ws_out_u8b.as<uint8_t>(), nullptr, pb, pe);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, hit, ctx->ws_out_u8b.p, (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_obstacle_sweep(rrtx_ctx *ctx, int obstacle, double search_range, double robot_radius, int32_t *edge_ids,
                        int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  const int m = (int)ctx->sph_active.size();
  if (obstacle < 0 || obstacle >= m) return fail(ctx, RRTX_E_INVALID, "obstacle_sweep: obstacle %d out of range (%d spheres)", obstacle, m);
  if (cap < 0 || (cap > 0 && !edge_ids)) return fail(ctx, RRTX_E_INVALID, "obstacle_sweep: bad arguments");
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "obstacle_sweep on an empty tree");
  if (ctx->dim != 3) return fail(ctx, RRTX_E_STATE, "obstacle_sweep is the SimpleEdge (dim=3) path");
  const double *c = &ctx->sph[4 * (size_t)obstacle];
  const SweepObs o = sweep_obs(c, robot_radius, search_range, ctx->sph_active[obstacle] != 0);
  const int64_t dcap = cap > 0 ? cap : 1;
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)dcap));
  long long *total_dev = nullptr;
  int rc = launch_obstacle_sweep(ctx, c, o.thr_lt, o.thr_gt, o.ob, o.active, ctx->ws_out_i32.as<int32_t>(), cap, &total_dev);
  if (rc) return rc;
  int64_t total = 0;
  if ((rc = sweep_ids_out(ctx, "obstacle_sweep", "colliding edges", total_dev, edge_ids, cap, needed, &total))) return rc;
  if (total > 0) RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// rrtx_obstacle_sweep_batch (fn, release = false; apply: block the rows) and rrtx_obstacle_release_batch (release = true;
// apply: unblock them)
static int sphere_burst_host(rrtx_ctx *ctx, const char *fn, bool release, const int32_t *obstacles, int k,
                             const double *search_range, double robot_radius, int apply, int64_t *offsets, int32_t *edge_ids,
                             int64_t cap, int64_t *needed) {
  const int m = (int)ctx->sph_active.size();
  if (k < 0 || k > 65536 || !offsets || (k > 0 && (!obstacles || !search_range)) || cap < 0 || (cap > 0 && !edge_ids))
    return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  for (int j = 0; j < k; ++j)
    if (obstacles[j] < 0 || obstacles[j] >= m)
      return fail(ctx, RRTX_E_INVALID, "%s: obstacle %d (entry %d) out of range (%d spheres)", fn, obstacles[j], j, m);
  if (needed) *needed = 0;
  if (k == 0) { offsets[0] = 0; return RRTX_OK; }
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "%s on an empty tree", fn);
  if (ctx->dim != 3) return fail(ctx, RRTX_E_STATE, "%s is the SimpleEdge (dim=3) path", fn);
  if (ctx->ge_n == 0) { std::fill(offsets, offsets + k + 1, (int64_t)0); return RRTX_OK; }
  // per obstacle what rrtx_obstacle_sweep hands its launcher; a leaving obstacle is taken as in use whatever its flag
  // says (the reference marks it unused before its loop, R/DRRT_Q.jl:3302)
  ctx->swb_tab_host.resize((size_t)k);
  for (int j = 0; j < k; ++j)
    ctx->swb_tab_host[(size_t)j] = sweep_obs(&ctx->sph[4 * (size_t)obstacles[j]], robot_radius, search_range[j],
                                             release || ctx->sph_active[obstacles[j]]);
  int rc;
  if (release) {
    // the staying spheres: the packed in-use records of the edge checks, less the positions that leave
    if ((rc = sync_spheres(ctx, robot_radius))) return rc;
    std::vector<uint8_t> leaves((size_t)m, 0);
    for (int j = 0; j < k; ++j) leaves[(size_t)obstacles[j]] = 1;
    const std::vector<int32_t> pos = active_positions(ctx->sph_active);
    ctx->rel_stay_host.assign(pos.size(), 0);
    for (size_t a = 0; a < pos.size(); ++a) ctx->rel_stay_host[a] = leaves[(size_t)pos[a]] ? 0 : 1;
  }
  const int64_t dcap = cap > 0 ? cap : 1;
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)dcap));
  long long *total_dev = nullptr;
  if ((rc = launch_sphere_burst(ctx, k, release, ctx->ws_out_i32.as<int32_t>(), cap, &total_dev))) return rc;
  RRTX_HIP(ctx, copy_out(ctx, offsets, ctx->ws_swb_off.p, sizeof(int64_t) * (size_t)(k + 1)));
  int64_t total = 0;
  if ((rc = sweep_ids_out(ctx, fn, release ? "freed edges" : "colliding edges", total_dev, edge_ids, cap, needed, &total))) return rc;
  if (total > 0) {
    // addNewObstacle's dist = Inf / removeObstacle's dist = distOriginal for every id of every row, where the rows are
    if (apply && (rc = launch_graph_block_dev(ctx, release, ctx->ws_out_i32.as<int32_t>(), total))) return rc;
    RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return RRTX_OK;
}

int rrtx_obstacle_sweep_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, const double *search_range,
                              double robot_radius, int block, int64_t *offsets, int32_t *edge_ids, int64_t cap,
                              int64_t *needed) {
  CHECK_CTX(ctx);
  return sphere_burst_host(ctx, "obstacle_sweep_batch", false, obstacles, k, search_range, robot_radius, block, offsets, edge_ids, cap, needed);
}

int rrtx_obstacle_release_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, const double *search_range,
                                double robot_radius, int unblock, int64_t *offsets, int32_t *edge_ids, int64_t cap,
                                int64_t *needed) {
  CHECK_CTX(ctx);
  return sphere_burst_host(ctx, "obstacle_release_batch", true, obstacles, k, search_range, robot_radius, unblock, offsets, edge_ids, cap, needed);
}

static int points_check_args(rrtx_ctx *ctx, int kind, const double *p, int64_t np, const uint8_t *unsafe) {
  if (np < 0 || (np > 0 && (!p || !unsafe)) || (kind != 0 && kind != 1))
    return fail(ctx, RRTX_E_INVALID, "points_check: bad arguments");
  return RRTX_OK;
}

int rrtx_points_check_dev(rrtx_ctx *ctx, int kind, const double *p, int64_t np, double robot_radius, int quick,
                          uint8_t *unsafe, double *clearance) {
  CHECK_CTX(ctx);
  int rc = points_check_args(ctx, kind, p, np, unsafe);
  if (rc) return rc;
  if (kind == 0) return launch_points_spheres(ctx, p, np, robot_radius, quick, unsafe, clearance);
  return launch_points_polygons(ctx, p, np, robot_radius, unsafe, clearance);
}

int rrtx_points_check(rrtx_ctx *ctx, int kind, const double *p, int64_t np, double robot_radius, int quick,
                      uint8_t *unsafe, double *clearance) {
  CHECK_CTX(ctx);
  int rc = points_check_args(ctx, kind, p, np, unsafe);
  if (rc || np == 0) return rc;
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q, p, sizeof(double) * (size_t)np * ctx->dim));
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure((size_t)np));
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * (size_t)np));
  // (no certificate wanted: the polygon check then only walks the obstacles near each point)
  rc = rrtx_points_check_dev(ctx, kind, ctx->ws_q.as<double>(), np, robot_radius, quick,
                             ctx->ws_out_u8a.as<uint8_t>(), clearance ? ctx->ws_out_f64.as<double>() : nullptr);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, unsafe, ctx->ws_out_u8a.p, (size_t)np));
  RRTX_HIP(ctx, copy_out(ctx, clearance, ctx->ws_out_f64.p, sizeof(double) * (size_t)np));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// ---- steering -------------------------------------------------------------------------------
int rrtx_simple_steer(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double *dist, double *wdist) {
  CHECK_CTX(ctx);
  if (ne < 0 || (ne > 0 && (!s || !g))) return fail(ctx, RRTX_E_INVALID, "simple_steer: bad arguments");
  if (ne == 0) return RRTX_OK;
  RRTX_HIP(ctx, stage_pair(ctx, s, g, sizeof(double) * (size_t)ne * ctx->dim));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * (size_t)ne));
  int rc = launch_simple_steer(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, ctx->ws_out_dist.as<double>(),
                               ctx->ws_out_f64.as<double>());
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, dist, ctx->ws_out_dist.p, sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, wdist, ctx->ws_out_f64.p, sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

static int dubins_common(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                         double robot_radius, bool check, double *cost, uint8_t *word, uint8_t *hit,
                         int32_t *traj_len) {
  if (ne < 0 || (ne > 0 && (!s || !g || !cost)) || (check && ne > 0 && !hit))
    return fail(ctx, RRTX_E_INVALID, "dubins: bad arguments");
  if (ne == 0) return RRTX_OK;
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "Dubins steering needs a dim=4 [x y t theta] context");
  RRTX_HIP(ctx, stage_pair(ctx, s, g, sizeof(double) * (size_t)ne * 4));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure(3 * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_u8b.ensure((size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)ne));
  int rc;
  if (check)
    rc = launch_dubins_edges_check(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, r_min, robot_radius,
                                   ctx->ws_out_dist.as<double>(), ctx->ws_out_u8a.as<uint8_t>(),
                                   ctx->ws_out_u8b.as<uint8_t>(), ctx->ws_out_i32.as<int32_t>());
  else
    rc = launch_dubins_steer(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, r_min,
                             ctx->ws_out_dist.as<double>(), ctx->ws_out_u8a.as<uint8_t>());
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, cost, ctx->ws_out_dist.p, sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, word, ctx->ws_out_u8a.p, 3 * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, hit, ctx->ws_out_u8b.p, (size_t)ne));                  // (null unless check)
  RRTX_HIP(ctx, copy_out(ctx, traj_len, ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_dubins_steer(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min, double *cost,
                      uint8_t *word) {
  CHECK_CTX(ctx);
  return dubins_common(ctx, s, g, ne, r_min, 0.0, false, cost, word, nullptr, nullptr);
}

int rrtx_set_dubins_velocity(rrtx_ctx *ctx, double v_min, double v_max) {
  CHECK_CTX(ctx);
  ctx->dubins_vmin = v_min;
  ctx->dubins_vmax = v_max;
  return RRTX_OK;
}

int rrtx_dubins_steer_full(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min, double *dist,
                           double *wdist, double *velocity, uint8_t *word, uint8_t *valid_move) {
  CHECK_CTX(ctx);
  if (ne < 0 || (ne > 0 && (!s || !g))) return fail(ctx, RRTX_E_INVALID, "dubins_steer_full: bad arguments");
  if (ne == 0) return RRTX_OK;
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "Dubins steering needs a dim=4 [x y t theta] context");
  RRTX_HIP(ctx, stage_pair(ctx, s, g, sizeof(double) * (size_t)ne * 4));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * 3 * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure(4 * (size_t)ne));
  double *d_dist = ctx->ws_out_dist.as<double>(), *d_w = d_dist + ne, *d_v = d_w + ne;
  uint8_t *d_word = ctx->ws_out_u8a.as<uint8_t>(), *d_valid = d_word + 3 * (size_t)ne;
  int rc = launch_dubins_steer(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, r_min, d_dist, d_word, d_w, d_v,
                               d_valid);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, dist, d_dist, sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, wdist, d_w, sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, velocity, d_v, sizeof(double) * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, word, d_word, 3 * (size_t)ne));
  RRTX_HIP(ctx, copy_out(ctx, valid_move, d_valid, (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_dubins_edges_check(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                            double robot_radius, double *cost, uint8_t *word, uint8_t *hit, int32_t *traj_len) {
  CHECK_CTX(ctx);
  return dubins_common(ctx, s, g, ne, r_min, robot_radius, true, cost, word, hit, traj_len);
}

int rrtx_dubins_trajectory(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                           int64_t *traj_off, double *traj_xy, int cols_in, int64_t cap_rows, int64_t *needed_rows) {
  CHECK_CTX(ctx);
  if (ne < 0 || cap_rows < 0 || (ne > 0 && (!s || !g || !traj_off)) || (cap_rows > 0 && !traj_xy))
    return fail(ctx, RRTX_E_INVALID, "dubins_trajectory: bad arguments");
  if (cols_in != (ctx->opt_space_has_time ? 3 : 2))
    return fail(ctx, RRTX_E_INVALID, "dubins_trajectory: rows are %d doubles wide in this context (RRTX_OPT_SPACE_HAS_TIME = %d), "
                "the caller's buffer was sized for %d", ctx->opt_space_has_time ? 3 : 2, ctx->opt_space_has_time ? 1 : 0, cols_in);
  if (ne == 0) { if (needed_rows) *needed_rows = 0; if (traj_off) traj_off[0] = 0; return RRTX_OK; }
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "Dubins steering needs a dim=4 [x y t theta] context");
  RRTX_HIP(ctx, stage_pair(ctx, s, g, sizeof(double) * (size_t)ne * 4));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)ne));
  // pass 1: rows per edge
  int rc = launch_dubins_trajectory(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, r_min, nullptr, nullptr, 0,
                                    ctx->ws_out_i32.as<int32_t>());
  if (rc) return rc;
  std::vector<int32_t> len((size_t)ne);
  RRTX_HIP(ctx, copy_out(ctx, len.data(), ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  traj_off[0] = 0;
  for (int64_t i = 0; i < ne; ++i) traj_off[i + 1] = traj_off[i] + len[(size_t)i];
  const int64_t total = traj_off[ne];
  if ((rc = check_capacity(ctx, "dubins_trajectory", "rows", total, cap_rows, needed_rows))) return rc;
  if (total == 0) return RRTX_OK;
  // pass 2: write the polylines
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_out_off, traj_off, sizeof(int64_t) * ((size_t)ne + 1)));
  const size_t cols = ctx->opt_space_has_time ? 3 : 2;      // (x, y) or, in a space with time, (x, y, t)
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * cols * (size_t)total));
  rc = launch_dubins_trajectory(ctx, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), ne, r_min,
                                ctx->ws_out_off.as<int64_t>(), ctx->ws_out_f64.as<double>(), total, nullptr);
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, traj_xy, ctx->ws_out_f64.p, sizeof(double) * cols * (size_t)total));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

int rrtx_detmath_eval(rrtx_ctx *ctx, int op, const double *x, const double *y, int64_t n, double *out) {
  CHECK_CTX(ctx);
  if (n < 0 || op < 0 || op > 3 || (n > 0 && (!x || !out)) || (op == 2 && n > 0 && !y))
    return fail(ctx, RRTX_E_INVALID, "detmath_eval: bad arguments");
  if (n == 0) return RRTX_OK;
  const size_t pb = sizeof(double) * (size_t)n;
  RRTX_HIP(ctx, stage_pair(ctx, x, y ? y : x, pb));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(pb));
  int rc = launch_detmath_eval(ctx, op, ctx->ws_q.as<double>(), ctx->ws_q2.as<double>(), n, ctx->ws_out_dist.as<double>());
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, out, ctx->ws_out_dist.p, pb));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// ---- fused extend() preamble ------------------------------------------------------------------
// what every call of the family that returns a CSR refuses first; lists: every per-entry array it requires is given
static int extend_csr_args(rrtx_ctx *ctx, const char *fn, const double *q, int nq, const int64_t *offsets, int64_t cap, bool lists) {
  if (nq < 0 || cap < 0 || (nq > 0 && (!q || !offsets)) || (cap > 0 && !lists)) return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  return RRTX_OK;
}
// ... and what its host form answers for an empty batch
static int extend_empty(int64_t *offsets, int64_t *needed) {
  if (needed) *needed = 0;
  if (offsets) offsets[0] = 0;
  return RRTX_OK;
}
static int extend_candidates_args(rrtx_ctx *ctx, const double *q, int nq, const int64_t *offsets, const int32_t *idx,
                                  const double *cost, const uint8_t *hit_out, const uint8_t *hit_in, int64_t cap) {
  return extend_csr_args(ctx, "extend_candidates", q, nq, offsets, cap, idx && cost && hit_out && hit_in);
}

int rrtx_extend_candidates_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                               int64_t *offsets, int32_t *idx, double *cost, uint8_t *hit_out, uint8_t *hit_in,
                               int64_t cap, int64_t *needed_dev, int32_t *nearest_idx, double *nearest_dist,
                               uint8_t *sample_unsafe) {
  CHECK_CTX(ctx);
  int rc = extend_candidates_args(ctx, q, nq, offsets, idx, cost, hit_out, hit_in, cap);
  if (rc) return rc;
  if (ctx->dim != 3) return fail(ctx, RRTX_E_STATE, "extend_candidates is the SimpleEdge (dim=3) path");
  if (ctx->n_wraps != 0)
    return fail(ctx, RRTX_E_STATE, "extend_candidates reads kdFindNearest off the range lists, which is only valid "
                                   "without wrapped dimensions (use rrtx_extend_candidates_dubins / the separate calls)");
  if (nq == 0) return RRTX_OK;
  const bool want_nearest = nearest_idx && nearest_dist;
  // nearest falls out of the radius lists (kdFindNearest's answer lies inside the ball whenever the
  // ball is non-empty); a sample with an empty ball is answered by an expanding search on the device
  // (kernels_finish.hip), so no -1 reaches the caller.
  if (ctx->opt_extend_polygons) {
    RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)(cap > 0 ? cap : 1)));
    rc = launch_nn_radius(ctx, q, nullptr, r, nq, offsets, idx, cost, cap, needed_dev,
                              ctx->ws_owner.as<int32_t>(), want_nearest ? nearest_idx : nullptr,
                              want_nearest ? nearest_dist : nullptr);
    if (rc) return rc;
    return launch_candidate_edges_polygons(ctx, q, nq, offsets, idx, ctx->ws_owner.as<int32_t>(), cap, robot_radius,
                                           hit_out, hit_in, sample_unsafe, (r >= 0.0) ? r : -1.0);
  }
  // sphere list: in the culled search the sample pass and both directed edges of every neighbour are
  // decided where the neighbour is found (kernels_nn.hip, TileEmit) and the finish kernel hands out
  // the flags; the other search paths (small trees, culling off) run the two kernels of their own
  rc = sync_spheres(ctx, robot_radius);
  if (rc) return rc;
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)(cap > 0 ? cap : 1)));
  ExtendFuse ef;
  ef.r = (r >= 0.0) ? r : -1.0;
  ef.hit_out = hit_out; ef.hit_in = hit_in; ef.sample_unsafe = sample_unsafe;
  ef.fused = false;
  rc = launch_nn_radius(ctx, q, nullptr, r, nq, offsets, idx, cost, cap, needed_dev, ctx->ws_owner.as<int32_t>(),
                        want_nearest ? nearest_idx : nullptr, want_nearest ? nearest_dist : nullptr, &ef);
  if (rc || ef.fused) return rc;
  return launch_candidate_edges(ctx, q, nq, offsets, idx, ctx->ws_owner.as<int32_t>(), cap, robot_radius, hit_out,
                                hit_in, (r >= 0.0) ? r : -1.0, sample_unsafe);
}

// The samples of a batch among themselves into L, nq > 0: the join, then both directed edges of every entry by the
// kernels of the preamble: the "near" end of entry e is row idx[e] of the sample table instead of a node; the per-sample
// obstacle lists are built for this batch and ball.  A dim = 4 context: [x y t theta] and Dubins edges.
// (dim decides the join and the edge type; extend_self_args / extend_self_dubins_args have refused the other dim, so it
// agrees with the `dubins` flag by which extend_csr_host chose the columns)
static int extend_self_lists(rrtx_ctx *ctx, const Lists &L, const double *q, int nq, double r, double robot_radius, double r_min,
                             const uint8_t *skip) {
  NearTable table;
  int rc = ctx->dim == 4 ? launch_self_join_dubins(ctx, L, q, nq, r, skip, &table) : launch_self_join(ctx, L, q, nq, r, skip, &table);
  return rc ? rc : launch_list_edges(ctx, L, q, nq, robot_radius, r_min, r, table);
}

// The host form of the calls that return a CSR, after their own refusals.  Everything that is per sample sits in ONE small
// device block (CandidatesBlock), so that it leaves in one transfer; the per-entry arrays follow once the count is known.
// Small transfers go through the context's pinned arena, large ones straight to the caller.  self: the _self calls, which
// take skip and have the CSR prefix of the block alone; dubins: three double columns and the words.
static int extend_csr_host(rrtx_ctx *ctx, const char *fn, bool self, bool dubins, const double *q, int nq, double r,
                           double robot_radius, double r_min, const uint8_t *skip, int64_t *offsets, const ListsOut &to, int64_t cap,
                           int64_t *needed, int32_t *nearest_idx = nullptr, double *nearest_dist = nullptr,
                           uint8_t *sample_unsafe = nullptr) {
  if (nq == 0) return extend_empty(offsets, needed);
  const CandidatesBlock B{(size_t)nq};
  const size_t blk_bytes = self ? B.csr_bytes : B.bytes;
  const size_t q_bytes = sizeof(double) * (size_t)nq * ctx->dim, skip_bytes = skip ? (size_t)nq : 0;
  Lists L;
  int rc = neighbour_lists(ctx, cap, dubins ? 3 : 1, dubins, &L);
  if (rc) return rc;
  RRTX_HIP(ctx, ctx->ws_out_off.ensure(blk_bytes));
  if ((rc = arena_begin(ctx, small_in(q_bytes) + small_in(skip_bytes) + block_need(blk_bytes) + lists_need(to, cap)))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_q, q, q_bytes))) return rc;
  if (skip && (rc = stage_in_small(ctx, ctx->ws_q2, skip, skip_bytes))) return rc;
  const double *q_dev = ctx->ws_q.as<double>();
  const uint8_t *skip_dev = skip ? ctx->ws_q2.as<uint8_t>() : nullptr;
  char *blk = ctx->ws_out_off.as<char>(), *host_blk;
  const bool want_nearest = nearest_idx && nearest_dist;
  L.offsets = B.offsets.in(blk); L.count = B.count.in(blk);
  if (self)
    rc = extend_self_lists(ctx, L, q_dev, nq, r, robot_radius, r_min, skip_dev);
  else      // (the SimpleEdge preamble keeps its way through the public positional form)
    rc = rrtx_extend_candidates_dev(ctx, q_dev, nq, r, robot_radius, L.offsets, L.idx, L.key, L.e.hit_out, L.e.hit_in, cap,
                                    L.count, want_nearest ? B.nearest_idx.in(blk) : nullptr,
                                    want_nearest ? B.nearest_dist.in(blk) : nullptr,
                                    sample_unsafe ? B.sample_unsafe.in(blk) : nullptr);
  if (rc) return rc;
  if ((rc = block_down(ctx, fn, blk, blk_bytes, &host_blk))) return rc;
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  B.offsets.to(offsets, host_blk);
  const int64_t total = *B.count.in(host_blk);
  if (!self) ctx->last_neighbors = total;
  if ((rc = check_capacity(ctx, fn, "neighbours", total, cap, needed))) return rc;
  if ((rc = lists_down(ctx, L, total, to))) return rc;
  // (the per-sample results are copied out of the arena while the per-entry transfers are in flight)
  B.sample_unsafe.to(sample_unsafe, host_blk);
  if (want_nearest) {
    B.nearest_dist.to(nearest_dist, host_blk);
    B.nearest_idx.to(nearest_idx, host_blk);
  }
  if ((rc = lists_finish(ctx, total))) return rc;
  return want_nearest ? nearest_fallback(ctx, q, nq, ctx->dim, nearest_idx, nearest_dist) : RRTX_OK;
}

int rrtx_extend_candidates(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius, int64_t *offsets,
                           int32_t *idx, double *cost, uint8_t *hit_out, uint8_t *hit_in, int64_t cap,
                           int64_t *needed, int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe) {
  CHECK_CTX(ctx);
  int rc = extend_candidates_args(ctx, q, nq, offsets, idx, cost, hit_out, hit_in, cap);
  if (rc) return rc;
  return extend_csr_host(ctx, "extend_candidates", false, false, q, nq, r, robot_radius, 0.0, nullptr, offsets,
                         ListsOut{idx, cost, nullptr, nullptr, nullptr, nullptr, hit_out, hit_in}, cap, needed, nearest_idx,
                         nearest_dist, sample_unsafe);
}

// ---- the samples of one extend batch among themselves (kernels_self.hip) ---------------------------
// (what rrtx_extend_candidates refuses, with its codes and before anything is staged)
static int extend_self_args(rrtx_ctx *ctx, const double *q, int nq, const int64_t *offsets, const int32_t *idx,
                            const double *cost, const uint8_t *hit_out, const uint8_t *hit_in, int64_t cap) {
  int rc = extend_csr_args(ctx, "extend_candidates_self", q, nq, offsets, cap, idx && cost && hit_out && hit_in);
  if (rc) return rc;
  if (ctx->dim != 3) return fail(ctx, RRTX_E_STATE, "extend_candidates_self is the SimpleEdge (dim=3) path");
  if (ctx->n_wraps != 0)
    return fail(ctx, RRTX_E_STATE, "extend_candidates_self completes the lists of rrtx_extend_candidates, which needs a "
                                   "space without wrapped dimensions");
  if (nq >= (1 << 30)) return fail(ctx, RRTX_E_INVALID, "extend_candidates_self: at most 2^30 - 1 samples per call");
  return RRTX_OK;
}

int rrtx_extend_candidates_self_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                    const uint8_t *skip, int64_t *offsets, int32_t *idx, double *cost,
                                    uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed_dev) {
  CHECK_CTX(ctx);
  int rc = extend_self_args(ctx, q, nq, offsets, idx, cost, hit_out, hit_in, cap);
  if (rc || nq == 0) return rc;
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)(cap > 0 ? cap : 1)));
  const Lists L{offsets, needed_dev, idx, ctx->ws_owner.as<int32_t>(), cost,
                EdgeCols{cost, cost, nullptr, nullptr, hit_out, hit_in}, cap};
  return extend_self_lists(ctx, L, q, nq, r, robot_radius, 0.0, skip);
}

int rrtx_extend_candidates_self(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                const uint8_t *skip, int64_t *offsets, int32_t *idx, double *cost, uint8_t *hit_out,
                                uint8_t *hit_in, int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  int rc = extend_self_args(ctx, q, nq, offsets, idx, cost, hit_out, hit_in, cap);
  if (rc) return rc;
  return extend_csr_host(ctx, "extend_candidates_self", true, false, q, nq, r, robot_radius, 0.0, skip, offsets,
                         ListsOut{idx, cost, nullptr, nullptr, nullptr, nullptr, hit_out, hit_in}, cap, needed);
}

// ---- the closestNode rule for an extend batch: k nearest earlier samples (kernels_self.hip) --------
static int extend_closest_args(rrtx_ctx *ctx, const double *q, int nq, int k, const int32_t *tree_idx, const int32_t *idx,
                               const double *cost, const uint8_t *hit_out, const uint8_t *hit_in, const int32_t *count,
                               const uint8_t *tree_hit_out, const uint8_t *tree_hit_in) {
  const int n_tree = (tree_idx ? 1 : 0) + (tree_hit_out ? 1 : 0) + (tree_hit_in ? 1 : 0);
  if (nq < 0 || k < 1 || k > RRTX_CLOSEST_SELF_MAX_K || (n_tree != 0 && n_tree != 3) ||
      (nq > 0 && (!q || !idx || !cost || !hit_out || !hit_in || !count)))
    return fail(ctx, RRTX_E_INVALID, "extend_closest_self: bad arguments");
  if (ctx->dim != 3) return fail(ctx, RRTX_E_STATE, "extend_closest_self is the SimpleEdge (dim=3) path");
  if (ctx->n_wraps != 0)
    return fail(ctx, RRTX_E_STATE, "extend_closest_self completes the lists of rrtx_extend_candidates, which needs a "
                                   "space without wrapped dimensions");
  if ((int64_t)nq * k >= (1ll << 30)) return fail(ctx, RRTX_E_INVALID, "extend_closest_self: at most 2^30 - 1 slots per call");
  return RRTX_OK;
}

int rrtx_extend_closest_self_dev(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius, const uint8_t *skip,
                                 const uint8_t *want, const int32_t *tree_idx, int32_t *idx, double *cost,
                                 uint8_t *hit_out, uint8_t *hit_in, int32_t *count, uint8_t *tree_hit_out,
                                 uint8_t *tree_hit_in) {
  CHECK_CTX(ctx);
  int rc = extend_closest_args(ctx, q, nq, k, tree_idx, idx, cost, hit_out, hit_in, count, tree_hit_out, tree_hit_in);
  if (rc || nq == 0) return rc;
  const int64_t slots = (int64_t)nq * k;
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)slots));
  const Lists L{nullptr, nullptr, idx, ctx->ws_owner.as<int32_t>(), cost,
                EdgeCols{cost, cost, nullptr, nullptr, hit_out, hit_in}, slots};
  return launch_closest_self(ctx, L, q, nq, k, robot_radius, skip, want, count,
                             TreeColumn{tree_idx, EdgeCols{nullptr, nullptr, nullptr, nullptr, tree_hit_out, tree_hit_in}});
}

int rrtx_extend_closest_self(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius, const uint8_t *skip,
                             const uint8_t *want, const int32_t *tree_idx, int32_t *idx, double *cost, uint8_t *hit_out,
                             uint8_t *hit_in, int32_t *count, uint8_t *tree_hit_out, uint8_t *tree_hit_in) {
  CHECK_CTX(ctx);
  int rc = extend_closest_args(ctx, q, nq, k, tree_idx, idx, cost, hit_out, hit_in, count, tree_hit_out, tree_hit_in);
  if (rc) return rc;
  if (nq == 0) return extend_empty(nullptr, nullptr);
  const size_t n = (size_t)nq, q_bytes = sizeof(double) * n * 3;
  const int64_t slots = (int64_t)nq * k;
  const ClosestInBlock I{n};
  const ClosestBlock B{n};
  const ListsOut to{idx, cost, nullptr, nullptr, nullptr, nullptr, hit_out, hit_in};
  Lists L;
  if ((rc = neighbour_lists(ctx, slots, 1, false, &L))) return rc;
  RRTX_HIP(ctx, ctx->ws_out_off.ensure(B.bytes));
  if ((rc = arena_begin(ctx, small_in(q_bytes) + block_need(I.bytes) + block_need(B.bytes) + lists_need(to, L.cap)))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_q, q, q_bytes))) return rc;
  if ((rc = closest_inputs_up(ctx, "extend_closest_self", I, skip, want, tree_idx))) return rc;
  char *in = ctx->ws_q2.as<char>(), *blk = ctx->ws_out_off.as<char>(), *host_blk;
  TreeColumn tree{};     // (tree_idx null: no tree column)
  if (tree_idx)
    tree = TreeColumn{I.tree_idx.in(in), EdgeCols{nullptr, nullptr, nullptr, nullptr, B.tree_hit_out.in(blk), B.tree_hit_in.in(blk)}};
  rc = launch_closest_self(ctx, L, ctx->ws_q.as<double>(), nq, k, robot_radius, skip ? I.skip.in(in) : nullptr,
                           want ? I.want.in(in) : nullptr, B.count.in(blk), tree);
  if (rc) return rc;
  // (no count to wait for: the block and the slots come down behind one another)
  if ((rc = block_down(ctx, "extend_closest_self", blk, B.bytes, &host_blk))) return rc;
  if ((rc = lists_down(ctx, L, slots, to))) return rc;
  if ((rc = lists_finish(ctx, slots))) return rc;
  B.count.to(count, host_blk);
  if (tree_idx) {
    B.tree_hit_out.to(tree_hit_out, host_blk);
    B.tree_hit_in.to(tree_hit_in, host_blk);
  }
  return RRTX_OK;
}

static int extend_dubins_args(rrtx_ctx *ctx, const double *q, int nq, const int64_t *offsets, const int32_t *idx,
                              const double *key, const double *cost_out, const double *cost_in, const uint8_t *hit_out,
                              const uint8_t *hit_in, int64_t cap) {
  if (nq < 0 || cap < 0 || (nq > 0 && (!q || !offsets)) ||
      (cap > 0 && (!idx || !key || !cost_out || !cost_in || !hit_out || !hit_in)))
    return fail(ctx, RRTX_E_INVALID, "extend_candidates_dubins: bad arguments");
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "extend_candidates_dubins needs a dim=4 [x y t theta] context");
  return RRTX_OK;
}

// The Dubins preamble into L, nq > 0: radius search, candidate Dubins edges, sample points, then the nearest scan under wraps.
static int extend_dubins_lists(rrtx_ctx *ctx, const Lists &L, const double *q, int nq, double r, double robot_radius, double r_min,
                               int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe) {
  const bool want_nearest = nearest_idx && nearest_dist;
  // with wrapped dimensions a list key is the distance to the copy that found the node FIRST
  // (addToRangeList), not the minimum over the copies, so kdFindNearest cannot be read off the list
  const bool nearest_from_list = want_nearest && ctx->n_wraps == 0;
  int rc = launch_nn_radius(ctx, q, nullptr, r, nq, L.offsets, L.idx, L.key, L.cap, L.count, L.owner,
                            nearest_from_list ? nearest_idx : nullptr, nearest_from_list ? nearest_dist : nullptr);
  if (rc) return rc;
  rc = launch_candidate_dubins(ctx, L, q, nq, r_min, robot_radius);
  if (rc) return rc;
  if (sample_unsafe) {
    rc = launch_points_polygons(ctx, q, nq, robot_radius, sample_unsafe, nullptr);
    if (rc) return rc;
  }
  if (want_nearest && !nearest_from_list) {
    rc = launch_nn_nearest(ctx, q, nq, nearest_idx, nearest_dist);
    if (rc) return rc;
  }
  return RRTX_OK;
}

int rrtx_extend_candidates_dubins_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                      double r_min, int64_t *offsets, int32_t *idx, double *key, double *cost_out,
                                      double *cost_in, uint8_t *word_out, uint8_t *word_in, uint8_t *hit_out,
                                      uint8_t *hit_in, int64_t cap, int64_t *needed_dev, int32_t *nearest_idx,
                                      double *nearest_dist, uint8_t *sample_unsafe) {
  CHECK_CTX(ctx);
  int rc = extend_dubins_args(ctx, q, nq, offsets, idx, key, cost_out, cost_in, hit_out, hit_in, cap);
  if (rc || nq == 0) return rc;
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)(cap > 0 ? cap : 1)));
  const Lists L{offsets, needed_dev, idx, ctx->ws_owner.as<int32_t>(), key,
                EdgeCols{cost_out, cost_in, word_out, word_in, hit_out, hit_in}, cap};
  return extend_dubins_lists(ctx, L, q, nq, r, robot_radius, r_min, nearest_idx, nearest_dist, sample_unsafe);
}

int rrtx_extend_candidates_dubins(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                  double r_min, int64_t *offsets, int32_t *idx, double *key, double *cost_out,
                                  double *cost_in, uint8_t *word_out, uint8_t *word_in, uint8_t *hit_out,
                                  uint8_t *hit_in, int64_t cap, int64_t *needed, int32_t *nearest_idx,
                                  double *nearest_dist, uint8_t *sample_unsafe) {
  CHECK_CTX(ctx);
  int rc = extend_dubins_args(ctx, q, nq, offsets, idx, key, cost_out, cost_in, hit_out, hit_in, cap);
  if (rc) return rc;
  if (nq == 0) { if (needed) *needed = 0; if (offsets) offsets[0] = 0; return RRTX_OK; }
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q, q, sizeof(double) * (size_t)nq * 4));
  const int64_t dcap = cap > 0 ? cap : 1;
  const bool want_nearest = nearest_idx && nearest_dist;
  RRTX_HIP(ctx, ctx->ws_out_off.ensure(sizeof(int64_t) * ((size_t)nq + 2)));
  RRTX_HIP(ctx, ctx->ws_out_idx.ensure(sizeof(int32_t) * (size_t)dcap));
  RRTX_HIP(ctx, ctx->ws_out_dist.ensure(sizeof(double) * 3 * (size_t)dcap));          // key, cost_out, cost_in
  RRTX_HIP(ctx, ctx->ws_out_u8a.ensure(8 * (size_t)dcap + (size_t)nq));                // words (3+3), hits (1+1), unsafe
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)nq));
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * (size_t)nq));
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)dcap));
  int64_t *off_dev = ctx->ws_out_off.as<int64_t>();
  int64_t *needed_dev = off_dev + nq + 1;
  double *key_dev = ctx->ws_out_dist.as<double>(), *co_dev = key_dev + dcap, *ci_dev = co_dev + dcap;
  uint8_t *wo_dev = ctx->ws_out_u8a.as<uint8_t>(), *wi_dev = wo_dev + 3 * dcap, *ho_dev = wi_dev + 3 * dcap,
          *hi_dev = ho_dev + dcap, *unsafe_dev = hi_dev + dcap;
  rc = rrtx_extend_candidates_dubins_dev(ctx, ctx->ws_q.as<double>(), nq, r, robot_radius, r_min, off_dev,
                                         ctx->ws_out_idx.as<int32_t>(), key_dev, co_dev, ci_dev, wo_dev, wi_dev, ho_dev,
                                         hi_dev, cap, needed_dev, want_nearest ? ctx->ws_out_i32.as<int32_t>() : nullptr,
                                         want_nearest ? ctx->ws_out_f64.as<double>() : nullptr,
                                         sample_unsafe ? unsafe_dev : nullptr);
  if (rc) return rc;
  int64_t total = 0;
  RRTX_HIP(ctx, copy_out(ctx, offsets, off_dev, sizeof(int64_t) * ((size_t)nq + 1)));
  RRTX_HIP(ctx, read_count(ctx, needed_dev, &total));
  ctx->last_neighbors = total;
  if ((rc = check_capacity(ctx, "extend_candidates_dubins", "neighbours", total, cap, needed))) return rc;
  const size_t n = (size_t)total;
  RRTX_HIP(ctx, copy_out(ctx, idx, ctx->ws_out_idx.p, sizeof(int32_t) * n));
  RRTX_HIP(ctx, copy_out(ctx, key, key_dev, sizeof(double) * n));
  RRTX_HIP(ctx, copy_out(ctx, cost_out, co_dev, sizeof(double) * n));
  RRTX_HIP(ctx, copy_out(ctx, cost_in, ci_dev, sizeof(double) * n));
  RRTX_HIP(ctx, copy_out(ctx, word_out, wo_dev, 3 * n));
  RRTX_HIP(ctx, copy_out(ctx, word_in, wi_dev, 3 * n));
  RRTX_HIP(ctx, copy_out(ctx, hit_out, ho_dev, n));
  RRTX_HIP(ctx, copy_out(ctx, hit_in, hi_dev, n));
  RRTX_HIP(ctx, copy_out(ctx, sample_unsafe, unsafe_dev, (size_t)nq));
  if (want_nearest) {
    RRTX_HIP(ctx, copy_out(ctx, nearest_idx, ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)nq));
    RRTX_HIP(ctx, copy_out(ctx, nearest_dist, ctx->ws_out_f64.p, sizeof(double) * (size_t)nq));
  }
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return want_nearest ? nearest_fallback(ctx, q, nq, 4, nearest_idx, nearest_dist) : RRTX_OK;
}

// ---- the samples of one Dubins extend batch among themselves (kernels_self.hip) ----------------------
// (what both forms refuse, before anything is staged: the join packs flags into the top two bits of the owner word)
static int extend_self_dubins_args(rrtx_ctx *ctx, const double *q, int nq, const int64_t *offsets, const int32_t *idx,
                                   const double *key, const double *cost_out, const double *cost_in, const uint8_t *hit_out,
                                   const uint8_t *hit_in, int64_t cap) {
  int rc = extend_dubins_args(ctx, q, nq, offsets, idx, key, cost_out, cost_in, hit_out, hit_in, cap);
  if (rc) return rc;
  if (nq >= (1 << 30)) return fail(ctx, RRTX_E_INVALID, "extend_candidates_self_dubins: at most 2^30 - 1 samples per call");
  return RRTX_OK;
}
int rrtx_extend_candidates_self_dubins_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                           double r_min, const uint8_t *skip, int64_t *offsets, int32_t *idx, double *key,
                                           double *cost_out, double *cost_in, uint8_t *word_out, uint8_t *word_in,
                                           uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed_dev) {
  CHECK_CTX(ctx);
  int rc = extend_self_dubins_args(ctx, q, nq, offsets, idx, key, cost_out, cost_in, hit_out, hit_in, cap);
  if (rc || nq == 0) return rc;
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)(cap > 0 ? cap : 1)));
  const Lists L{offsets, needed_dev, idx, ctx->ws_owner.as<int32_t>(), key,
                EdgeCols{cost_out, cost_in, word_out, word_in, hit_out, hit_in}, cap};
  return extend_self_lists(ctx, L, q, nq, r, robot_radius, r_min, skip);
}

int rrtx_extend_candidates_self_dubins(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                       double r_min, const uint8_t *skip, int64_t *offsets, int32_t *idx, double *key,
                                       double *cost_out, double *cost_in, uint8_t *word_out, uint8_t *word_in,
                                       uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  int rc = extend_self_dubins_args(ctx, q, nq, offsets, idx, key, cost_out, cost_in, hit_out, hit_in, cap);
  if (rc) return rc;
  return extend_csr_host(ctx, "extend_candidates_self_dubins", true, true, q, nq, r, robot_radius, r_min, skip, offsets,
                         ListsOut{idx, key, cost_out, cost_in, word_out, word_in, hit_out, hit_in}, cap, needed);
}

// ---- the closestNode rule for a Dubins extend batch: k nearest earlier samples in wrapped space (kernels_self.hip) ----
static int extend_closest_dubins_args(rrtx_ctx *ctx, const double *q, int nq, int k, const int32_t *tree_idx,
                                      const int32_t *idx, const double *key, const double *cost_out, const double *cost_in,
                                      const uint8_t *hit_out, const uint8_t *hit_in, const int32_t *count,
                                      const double *tree_cost_out, const double *tree_cost_in, const uint8_t *tree_hit_out,
                                      const uint8_t *tree_hit_in) {
  const int n_tree = (tree_idx ? 1 : 0) + (tree_cost_out ? 1 : 0) + (tree_cost_in ? 1 : 0) + (tree_hit_out ? 1 : 0) +
                     (tree_hit_in ? 1 : 0);
  if (nq < 0 || k < 1 || k > RRTX_CLOSEST_SELF_MAX_K || (n_tree != 0 && n_tree != 5) ||
      (nq > 0 && (!q || !idx || !key || !cost_out || !cost_in || !hit_out || !hit_in || !count)))
    return fail(ctx, RRTX_E_INVALID, "extend_closest_self_dubins: bad arguments");
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "extend_closest_self_dubins needs a dim=4 [x y t theta] context");
  if ((int64_t)nq * k >= (1ll << 30))
    return fail(ctx, RRTX_E_INVALID, "extend_closest_self_dubins: at most 2^30 - 1 slots per call");
  return RRTX_OK;
}

int rrtx_extend_closest_self_dubins_dev(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius, double r_min,
                                        const uint8_t *skip, const uint8_t *want, const int32_t *tree_idx, int32_t *idx,
                                        double *key, double *cost_out, double *cost_in, uint8_t *word_out,
                                        uint8_t *word_in, uint8_t *hit_out, uint8_t *hit_in, int32_t *count,
                                        double *tree_cost_out, double *tree_cost_in, uint8_t *tree_word_out,
                                        uint8_t *tree_word_in, uint8_t *tree_hit_out, uint8_t *tree_hit_in) {
  CHECK_CTX(ctx);
  int rc = extend_closest_dubins_args(ctx, q, nq, k, tree_idx, idx, key, cost_out, cost_in, hit_out, hit_in, count,
                                      tree_cost_out, tree_cost_in, tree_hit_out, tree_hit_in);
  if (rc || nq == 0) return rc;
  const int64_t slots = (int64_t)nq * k;
  RRTX_HIP(ctx, ctx->ws_owner.ensure(sizeof(int32_t) * (size_t)slots));
  const Lists L{nullptr, nullptr, idx, ctx->ws_owner.as<int32_t>(), key,
                EdgeCols{cost_out, cost_in, word_out, word_in, hit_out, hit_in}, slots};
  return launch_closest_self_dubins(ctx, L, q, nq, k, robot_radius, r_min, skip, want, count,
                                    TreeColumn{tree_idx, EdgeCols{tree_cost_out, tree_cost_in, tree_idx ? tree_word_out : nullptr,
                                                                  tree_idx ? tree_word_in : nullptr, tree_hit_out, tree_hit_in}});
}

int rrtx_extend_closest_self_dubins(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius, double r_min,
                                    const uint8_t *skip, const uint8_t *want, const int32_t *tree_idx, int32_t *idx,
                                    double *key, double *cost_out, double *cost_in, uint8_t *word_out, uint8_t *word_in,
                                    uint8_t *hit_out, uint8_t *hit_in, int32_t *count, double *tree_cost_out,
                                    double *tree_cost_in, uint8_t *tree_word_out, uint8_t *tree_word_in,
                                    uint8_t *tree_hit_out, uint8_t *tree_hit_in) {
  CHECK_CTX(ctx);
  int rc = extend_closest_dubins_args(ctx, q, nq, k, tree_idx, idx, key, cost_out, cost_in, hit_out, hit_in, count,
                                      tree_cost_out, tree_cost_in, tree_hit_out, tree_hit_in);
  if (rc) return rc;
  if (nq == 0) return extend_empty(nullptr, nullptr);
  const size_t n = (size_t)nq, q_bytes = sizeof(double) * n * 4;
  const int64_t slots = (int64_t)nq * k;
  const ClosestInBlock I{n};
  const ClosestDubinsBlock B{n};
  const ListsOut to{idx, key, cost_out, cost_in, word_out, word_in, hit_out, hit_in};
  Lists L;
  if ((rc = neighbour_lists(ctx, slots, 3, true, &L))) return rc;
  RRTX_HIP(ctx, ctx->ws_out_off.ensure(B.bytes));
  if ((rc = arena_begin(ctx, small_in(q_bytes) + block_need(I.bytes) + block_need(B.bytes) + lists_need(to, L.cap)))) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_q, q, q_bytes))) return rc;
  if ((rc = closest_inputs_up(ctx, "extend_closest_self_dubins", I, skip, want, tree_idx))) return rc;
  char *in = ctx->ws_q2.as<char>(), *blk = ctx->ws_out_off.as<char>(), *host_blk;
  TreeColumn tree{};     // (tree_idx null: no tree column)
  if (tree_idx)
    tree = TreeColumn{I.tree_idx.in(in), EdgeCols{B.tree_cost_out.in(blk), B.tree_cost_in.in(blk), B.tree_word_out.in(blk),
                                                  B.tree_word_in.in(blk), B.tree_hit_out.in(blk), B.tree_hit_in.in(blk)}};
  rc = launch_closest_self_dubins(ctx, L, ctx->ws_q.as<double>(), nq, k, robot_radius, r_min, skip ? I.skip.in(in) : nullptr,
                                  want ? I.want.in(in) : nullptr, B.count.in(blk), tree);
  if (rc) return rc;
  // (no count to wait for: the block and the slots come down behind one another)
  if ((rc = block_down(ctx, "extend_closest_self_dubins", blk, B.bytes, &host_blk))) return rc;
  if ((rc = lists_down(ctx, L, slots, to))) return rc;
  if ((rc = lists_finish(ctx, slots))) return rc;
  B.count.to(count, host_blk);
  if (tree_idx) {
    B.tree_cost_out.to(tree_cost_out, host_blk);
    B.tree_cost_in.to(tree_cost_in, host_blk);
    B.tree_word_out.to(tree_word_out, host_blk);
    B.tree_word_in.to(tree_word_in, host_blk);
    B.tree_hit_out.to(tree_hit_out, host_blk);
    B.tree_hit_in.to(tree_hit_in, host_blk);
  }
  return RRTX_OK;
}

int rrtx_pack_hits_dev(rrtx_ctx *ctx, const uint8_t *hit_out, const uint8_t *hit_in, const int64_t *n_valid_dev,
                       int64_t cap, uint64_t *words) {
  CHECK_CTX(ctx);
  if (cap < 0 || (cap > 0 && (!hit_out || !hit_in || !n_valid_dev || !words)))
    return fail(ctx, RRTX_E_INVALID, "pack_hits: bad arguments");
  return launch_pack_hits(ctx, hit_out, hit_in, n_valid_dev, cap, words);
}

// ---- parent and rewire selection over the extend lists (kernels_select.hip) -----------------------
// (the selection over lists on the device, rrtLMC a device array or null for the context's own: shared by the _dev entry
// point and rrtx_extend_select, which runs it inside its own call)
static int select_over_lists(rrtx_ctx *ctx, SelectLaunch S) {
  if (!S.lmc) {
    Lmc own;
    if (int rc = resolve_lmc(ctx, nullptr, &own)) return rc;
    S.lmc = own.dev; S.n_lmc = own.n;
  }
  return launch_select(ctx, S);
}

int rrtx_extend_select_dev(rrtx_ctx *ctx, int nq, const int64_t *offsets, const int32_t *idx, const double *cost_out,
                           const double *cost_in, const uint8_t *hit_out, const uint8_t *hit_in,
                           const int64_t *n_valid_dev, int64_t cap, const uint8_t *sample_unsafe, const double *lmc,
                           int32_t *parent_idx, int64_t *parent_entry, double *lmc_new, uint8_t *status,
                           int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap,
                           int64_t *rw_needed_dev) {
  CHECK_CTX(ctx);
  if (nq < 0 || cap < 0 || rw_cap < 0 || !offsets || !rw_offsets || !rw_needed_dev ||
      (nq > 0 && (!parent_idx || !parent_entry || !lmc_new || !status)) ||
      (cap > 0 && (!idx || !cost_out || !cost_in || !hit_out || !hit_in)) || (rw_cap > 0 && (!rw_node || !rw_value)))
    return fail(ctx, RRTX_E_INVALID, "extend_select: bad arguments");
  const ListsRO L{offsets, n_valid_dev, idx, nullptr, nullptr, {cost_out, cost_in, nullptr, nullptr, hit_out, hit_in}, cap};
  return select_over_lists(ctx, SelectLaunch{nq, L, sample_unsafe, lmc, ctx->n_nodes, parent_idx, parent_entry, lmc_new, status,
                                             rw_offsets, rw_node, rw_value, rw_cap, rw_needed_dev});
}

int rrtx_node_cost_set(rrtx_ctx *ctx, int64_t first_index, const double *lmc, int64_t n) {
  CHECK_CTX_KEEP(ctx);
  if (n < 0 || first_index < 0 || (n > 0 && !lmc)) return fail(ctx, RRTX_E_INVALID, "node_cost_set: bad arguments");
  if (first_index > ctx->n_nodes || n > ctx->n_nodes - first_index)
    return fail(ctx, RRTX_E_INVALID, "node_cost_set: nodes %lld .. %lld of %lld", (long long)first_index,
                (long long)(first_index + n), (long long)ctx->n_nodes);
  int rc = node_cost_ensure(ctx);
  if (rc || n == 0) return rc;
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->node_lmc + first_index, lmc, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return RRTX_OK;
}

// (the lists a host-pointer select call may hand back: all or none, offsets null for none.  SimpleEdge has the one cost
// column, given as `key`; Dubins has key, cost_out and cost_in)
struct SelectListsOut { int64_t *offsets; ListsOut to; int64_t cap; int64_t *needed; };
// samples with an empty ball, resolved like nearest_fallback but through no entry point: the misses go up into ws_q2,
// the full scan answers into ws_out_i32 / ws_out_f64.  Neither those nor the scan's own workspaces (ws_slots, ws_copies*,
// ws_copy_meta, ws_scalars_nn, ws_recs, ws_partial) hold a list or the select block, so the held lists stay valid.
static int nearest_fallback_keep(rrtx_ctx *ctx, const double *q, int nq, int dim, int32_t *nearest_idx, double *nearest_dist) {
  std::vector<int> miss;
  for (int i = 0; i < nq; ++i) if (nearest_idx[i] < 0) miss.push_back(i);
  if (miss.empty() || ctx->n_nodes <= 0) return RRTX_OK;
  const int nm = (int)miss.size();
  std::vector<double> mq((size_t)nm * (size_t)dim);
  for (int k = 0; k < nm; ++k) std::memcpy(&mq[(size_t)k * dim], q + (size_t)miss[k] * dim, sizeof(double) * dim);
  std::vector<int32_t> mi((size_t)nm);
  std::vector<double> md((size_t)nm);
  RRTX_HIP(ctx, stage_in(ctx, ctx->ws_q2, mq.data(), sizeof(double) * mq.size()));
  RRTX_HIP(ctx, ctx->ws_out_i32.ensure(sizeof(int32_t) * (size_t)nm));
  RRTX_HIP(ctx, ctx->ws_out_f64.ensure(sizeof(double) * (size_t)nm));
  int rc = launch_nn_nearest(ctx, ctx->ws_q2.as<double>(), nm, ctx->ws_out_i32.as<int32_t>(), ctx->ws_out_f64.as<double>());
  if (rc) return rc;
  RRTX_HIP(ctx, copy_out(ctx, mi.data(), ctx->ws_out_i32.p, sizeof(int32_t) * (size_t)nm));
  RRTX_HIP(ctx, copy_out(ctx, md.data(), ctx->ws_out_f64.p, sizeof(double) * (size_t)nm));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < nm; ++k) { nearest_idx[miss[k]] = mi[k]; nearest_dist[miss[k]] = md[k]; }
  return RRTX_OK;
}

// The body rrtx_extend_select and rrtx_extend_select_dubins share: the extend preamble into lists the context owns,
// the selection over them, the per-sample block down in one transfer, then the rewire lists and (asked for) the
// neighbour lists.  dubins: the three double columns of neighbour_lists, else the one.  On success the context holds
// the lists.
static int extend_select_host(rrtx_ctx *ctx, const char *fn, bool dubins, const double *q, int nq, double r, double robot_radius,
                              double r_min, const double *lmc, int32_t *parent_idx, int64_t *parent_entry, double *lmc_new,
                              uint8_t *status, int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap,
                              int64_t *rw_needed, int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe,
                              const SelectListsOut &out) {
  const bool want_lists = out.offsets != nullptr;
  const int cols = dubins ? 3 : 1;
  if (nq == 0) {
    rw_offsets[0] = 0;
    if (rw_needed) *rw_needed = 0;
    if (want_lists) out.offsets[0] = 0;
    if (out.needed) *out.needed = 0;
    ctx->sel_hold_nq = 0; ctx->sel_hold_count = 0; ctx->sel_hold_cols = cols;
    return RRTX_OK;
  }
  // Everything that is per sample sits in ONE device block (SelectBlock), so that it leaves in one transfer: without
  // its tail, the list offsets, unless the caller wants the lists.
  const size_t n = (size_t)nq;
  const SelectBlock B{n};
  const size_t out_bytes = want_lists ? B.bytes : B.bytes_without_lists;
  const size_t q_bytes = sizeof(double) * n * (size_t)ctx->dim;
  int rc = arena_begin(ctx, small_in(q_bytes) + lmc_arena_need(ctx, lmc) + block_need(out_bytes) + out_need(rw_value, sizeof(double), rw_cap) +
                                out_need(rw_node, sizeof(int32_t), rw_cap) + (want_lists ? lists_need(out.to, out.cap) : 0));
  if (rc) return rc;
  if ((rc = stage_in_small(ctx, ctx->ws_q, q, q_bytes))) return rc;
  Lmc lmc_dev;
  if ((rc = resolve_lmc(ctx, lmc, &lmc_dev))) return rc;
  RRTX_HIP(ctx, ctx->ws_sel_blk.ensure(B.bytes));
  RRTX_HIP(ctx, ctx->ws_sel_rwn.ensure(sizeof(int32_t) * (size_t)(rw_cap > 0 ? rw_cap : 1)));
  RRTX_HIP(ctx, ctx->ws_sel_rwv.ensure(sizeof(double) * (size_t)(rw_cap > 0 ? rw_cap : 1)));
  char *blk = ctx->ws_sel_blk.as<char>();
  char *host_blk = arena_take(ctx, out_bytes);
  if (!host_blk) return fail(ctx, RRTX_E_NOMEM, "%s: staging arena", fn);
  const bool want_nearest = nearest_idx && nearest_dist;
  Lists lists;
  rc = with_neighbour_lists(ctx, fn, nq, 0, cols, B.offsets.in(blk), host_blk, B.counts.in(blk), out_bytes, [&](const Lists &L) {
    lists = L;
    int32_t *ni = want_nearest ? B.nearest_idx.in(blk) : nullptr;
    double *nd = want_nearest ? B.nearest_dist.in(blk) : nullptr;
    // (in a wrapped Dubins space the preamble ends with the full nearest scan: it writes the two columns of the select
    // block and its own search workspaces, never a list)
    int rc;
    if (dubins)
      rc = extend_dubins_lists(ctx, L, ctx->ws_q.as<double>(), nq, r, robot_radius, r_min, ni, nd, B.sample_unsafe.in(blk));
    else      // (the SimpleEdge preamble keeps its way through the public positional form)
      rc = rrtx_extend_candidates_dev(ctx, ctx->ws_q.as<double>(), nq, r, robot_radius, L.offsets, L.idx, L.key, L.e.hit_out,
                                      L.e.hit_in, L.cap, L.count, ni, nd, B.sample_unsafe.in(blk));
    if (rc) return rc;
    return select_over_lists(ctx, SelectLaunch{nq, read_only(L), B.sample_unsafe.in(blk), lmc_dev.dev, lmc_dev.n,
                                               B.parent_idx.in(blk), B.parent_entry.in(blk), B.lmc_new.in(blk), B.status.in(blk),
                                               B.rw_offsets.in(blk), ctx->ws_sel_rwn.as<int32_t>(),
                                               ctx->ws_sel_rwv.as<double>(), rw_cap, B.counts.in(blk) + 1});
  });
  if (rc) return rc;
  const int64_t total = B.counts.in(host_blk)[0], rw_total = B.counts.in(host_blk)[1];
  B.rw_offsets.to(rw_offsets, host_blk);
  B.parent_entry.to(parent_entry, host_blk);
  B.lmc_new.to(lmc_new, host_blk);
  B.parent_idx.to(parent_idx, host_blk);
  B.status.to(status, host_blk);
  B.sample_unsafe.to(sample_unsafe, host_blk);
  if (want_nearest) {
    B.nearest_dist.to(nearest_dist, host_blk);
    B.nearest_idx.to(nearest_idx, host_blk);
  }
  if (want_lists) B.offsets.to(out.offsets, host_blk);
  if (out.needed) *out.needed = total;
  if ((rc = check_capacity(ctx, fn, "rewire entries", rw_total, rw_cap, rw_needed))) return rc;
  if (want_lists && (rc = check_capacity(ctx, fn, "neighbours", total, out.cap, out.needed))) return rc;
  if ((rc = d2h(ctx, rw_value, ctx->ws_sel_rwv.p, sizeof(double) * (size_t)rw_total))) return rc;
  if ((rc = d2h(ctx, rw_node, ctx->ws_sel_rwn.p, sizeof(int32_t) * (size_t)rw_total))) return rc;
  if (want_lists && (rc = lists_down(ctx, lists, total, out.to))) return rc;
  if ((rc = lists_finish(ctx, rw_total + (want_lists ? total : 0)))) return rc;
  // Dubins without wrapped dimensions reads the nearest off the lists like SimpleEdge; its empty balls are resolved
  // here, before the record is set and through no entry point, so the hold is valid whatever the caller asked for
  if (dubins && want_nearest && (rc = nearest_fallback_keep(ctx, q, nq, ctx->dim, nearest_idx, nearest_dist))) return rc;
  // the lists stay for rrtx_graph_edges_append_selected (the SimpleEdge nearest fallback, when it has to search, drops
  // the record again: rrtx_nn_nearest writes their workspaces)
  ctx->sel_hold_nq = nq; ctx->sel_hold_count = total; ctx->sel_hold_cols = cols;
  return want_nearest && !dubins ? nearest_fallback(ctx, q, nq, ctx->dim, nearest_idx, nearest_dist) : RRTX_OK;
}

int rrtx_extend_select(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius, const double *lmc,
                       int32_t *parent_idx, int64_t *parent_entry, double *lmc_new, uint8_t *status,
                       int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap, int64_t *rw_needed,
                       int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe, int64_t *offsets,
                       int32_t *idx, double *cost, uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  const bool want_lists = offsets != nullptr;
  if (nq < 0 || rw_cap < 0 || !rw_offsets || (nq > 0 && (!q || !parent_idx || !parent_entry || !lmc_new || !status)) ||
      (rw_cap > 0 && (!rw_node || !rw_value)) ||
      (want_lists && (cap < 0 || (cap > 0 && (!idx || !cost || !hit_out || !hit_in)))))
    return fail(ctx, RRTX_E_INVALID, "extend_select: bad arguments");
  if (ctx->dim != 3) return fail(ctx, RRTX_E_STATE, "extend_select is the SimpleEdge (dim=3) path");
  return extend_select_host(ctx, "extend_select", false, q, nq, r, robot_radius, 0.0, lmc, parent_idx, parent_entry, lmc_new,
                            status, rw_offsets, rw_node, rw_value, rw_cap, rw_needed, nearest_idx, nearest_dist, sample_unsafe,
                            SelectListsOut{offsets, ListsOut{idx, cost, nullptr, nullptr, nullptr, nullptr, hit_out, hit_in}, cap, needed});
}

int rrtx_extend_select_dubins(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius, double r_min,
                              const double *lmc, int32_t *parent_idx, int64_t *parent_entry, double *lmc_new,
                              uint8_t *status, int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap,
                              int64_t *rw_needed, int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe,
                              int64_t *offsets, int32_t *idx, double *key, double *cost_out, double *cost_in,
                              uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed) {
  CHECK_CTX(ctx);
  const bool want_lists = offsets != nullptr;
  if (nq < 0 || rw_cap < 0 || !rw_offsets || (nq > 0 && (!q || !parent_idx || !parent_entry || !lmc_new || !status)) ||
      (rw_cap > 0 && (!rw_node || !rw_value)) ||
      (want_lists && (cap < 0 || (cap > 0 && (!idx || !key || !cost_out || !cost_in || !hit_out || !hit_in)))))
    return fail(ctx, RRTX_E_INVALID, "extend_select_dubins: bad arguments");
  if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "extend_select_dubins needs a dim=4 [x y t theta] context");
  return extend_select_host(ctx, "extend_select_dubins", true, q, nq, r, robot_radius, r_min, lmc, parent_idx, parent_entry,
                            lmc_new, status, rw_offsets, rw_node, rw_value, rw_cap, rw_needed, nearest_idx, nearest_dist,
                            sample_unsafe, SelectListsOut{offsets, ListsOut{idx, key, cost_out, cost_in, nullptr, nullptr, hit_out, hit_in}, cap, needed});
}

// ---- findNewTarget over a batch of poses (kernels_target.hip) ---------------------------------------
namespace {
int find_new_target(rrtx_ctx *ctx, const char *fn, bool dubins, const double *pose, int nq, const double *r0, int r_stride,
                    double r_max, double robot_radius, double r_min, const double *lmc, int32_t *target_idx,
                    double *edge_dist, double *cost_to_goal, double *radius_used, int32_t *rounds, uint8_t *status) {
  if (nq < 0 || (r_stride != 0 && r_stride != 1) ||
      (nq > 0 && (!pose || !r0 || !target_idx || !edge_dist || !cost_to_goal || !radius_used || !rounds || !status)))
    return fail(ctx, RRTX_E_INVALID, "%s: bad arguments", fn);
  if (dubins) {
    if (ctx->dim != 4) return fail(ctx, RRTX_E_STATE, "%s needs a dim=4 [x y t theta] context", fn);
  } else if (ctx->dim != 3 || ctx->n_wraps != 0) {
    return fail(ctx, RRTX_E_STATE, "%s is the SimpleEdge path: dim=3 without wrapped dimensions", fn);
  }
  if (!std::isfinite(r_max)) return fail(ctx, RRTX_E_INVALID, "%s: r_max must be finite", fn);
  for (int i = 0; i < (r_stride ? nq : std::min(nq, 1)); ++i)
    if (!std::isfinite(r0[i]) || !(r0[i] > 0.0) || !(r0[i] >= r_max * 0x1p-40))
      return fail(ctx, RRTX_E_INVALID, "%s: r0[%d] = %g is not a finite positive radius of at least r_max / 2^40", fn, i, r0[i]);
  if (ctx->n_nodes <= 0) return fail(ctx, RRTX_E_STATE, "%s on an empty tree", fn);
  if (nq == 0) return RRTX_OK;

  // One query block per round side (TargetQueryBlock), so that the first round's goes up in one transfer; one result
  // block (TargetResultBlock) whose results leave in one transfer at the end.
  const size_t n = (size_t)nq;
  const TargetQueryBlock Q{n, (size_t)ctx->dim};
  const TargetResultBlock R{n};
  int rc = arena_begin(ctx, Q.bytes + R.result_bytes + lmc_arena_need(ctx, lmc) + 1024);
  if (rc) return rc;
  RRTX_HIP(ctx, ctx->ws_tgt_blk[0].ensure(Q.bytes));
  RRTX_HIP(ctx, ctx->ws_tgt_blk[1].ensure(Q.bytes));
  RRTX_HIP(ctx, ctx->ws_tgt_res.ensure(R.bytes));
  RRTX_HIP(ctx, ctx->ws_out_off.ensure(sizeof(int64_t) * (n + 2)));
  char *up = arena_take(ctx, Q.bytes);
  char *host_res = arena_take(ctx, R.result_bytes);
  int64_t *host_hdr = reinterpret_cast<int64_t *>(arena_take(ctx, R.hdr.bytes()));
  if (!up || !host_res || !host_hdr) return fail(ctx, RRTX_E_NOMEM, "%s: staging arena", fn);
  std::memcpy(Q.pose.in(up), pose, Q.pose.bytes());
  for (int i = 0; i < nq; ++i) { Q.rad.in(up)[i] = r0[r_stride ? i : 0]; Q.slot.in(up)[i] = i; }
  fill_thresholds(r0, r_stride, nq, Q.thr.in(up), Q.thr.in(up) + n);
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_tgt_blk[0].p, up, Q.bytes, hipMemcpyHostToDevice, ctx->stream));
  Lmc lmc_dev;
  if ((rc = resolve_lmc(ctx, lmc, &lmc_dev))) return rc;
  char *res = ctx->ws_tgt_res.as<char>();
  int64_t *hdr_dev = R.hdr.in(res), *off_dev = ctx->ws_out_off.as<int64_t>();
  int n_act = nq, side = 0;
  int64_t room = 0;          // entries the coming round asks for beyond what the lists hold
  for (int round = 1; n_act > 0; ++round, side ^= 1) {
    if (round > 64) return fail(ctx, RRTX_E_STATE, "%s: %d poses still searching after 64 rounds", fn, n_act);
    char *cur = ctx->ws_tgt_blk[side].as<char>(), *nxt = ctx->ws_tgt_blk[side ^ 1].as<char>();
    const double *q_dev = Q.pose.in(cur);
    rc = with_neighbour_lists(ctx, fn, nq, room, dubins ? 3 : 1, off_dev, host_hdr, hdr_dev, R.hdr.bytes(), [&](const Lists &L) {
      int rc = launch_nn_radius(ctx, q_dev, Q.thr.in(cur), 0.0, n_act, L.offsets, L.idx, L.key, L.cap, L.count, L.owner);
      if (rc) return rc;
      // (r < 0: the radii differ from pose to pose, every obstacle is looked at)
      rc = launch_list_edges(ctx, L, q_dev, n_act, robot_radius, r_min, -1.0);
      if (rc) return rc;
      TargetRound T;
      T.n_act = n_act; T.nq = nq; T.round = round; T.dim = ctx->dim; T.r_max = r_max;
      T.offsets = L.offsets; T.idx = L.idx; T.cost = L.e.cost_out; T.hit_out = L.e.hit_out;
      T.n_valid = L.count; T.cap = (long long)L.cap;
      T.lmc = lmc_dev.dev; T.n_lmc = (long long)lmc_dev.n;
      T.q = q_dev; T.rad = Q.rad.in(cur); T.slot = Q.slot.in(cur);
      T.pending = R.pending.in(res);
      T.cost_to_goal = R.cost_to_goal.in(res); T.edge_dist = R.edge_dist.in(res); T.radius_used = R.radius_used.in(res);
      T.target_idx = R.target_idx.in(res); T.rounds = R.rounds.in(res); T.status = R.status.in(res);
      T.q_next = Q.pose.in(nxt); T.rad_next = Q.rad.in(nxt); T.thr_next = Q.thr.in(nxt); T.slot_next = Q.slot.in(nxt);
      T.hdr = hdr_dev;
      return launch_target_round(ctx, T);
    });
    if (rc) return rc;
    if (host_hdr[1] < 0 || host_hdr[1] > n_act) return fail(ctx, RRTX_E_STATE, "%s: round %d left %lld of %d poses", fn, round, (long long)host_hdr[1], n_act);
    n_act = (int)host_hdr[1];
    // twice the radius is eight times the ball: make room for what the poses that go on will find (at most every node each)
    const int64_t guess = std::min<int64_t>(host_hdr[2] * 8, (int64_t)n_act * ctx->n_nodes);
    room = guess > ctx->sel_list_cap ? guess + guess / 8 : 0;
  }
  RRTX_HIP(ctx, hipMemcpyAsync(host_res, res, R.result_bytes, hipMemcpyDeviceToHost, ctx->stream));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  R.cost_to_goal.to(cost_to_goal, host_res);
  R.edge_dist.to(edge_dist, host_res);
  R.radius_used.to(radius_used, host_res);
  R.target_idx.to(target_idx, host_res);
  R.rounds.to(rounds, host_res);
  R.status.to(status, host_res);
  return RRTX_OK;
}
}  // namespace

int rrtx_find_new_target(rrtx_ctx *ctx, const double *pose, int nq, const double *r0, int r_stride, double r_max,
                         double robot_radius, const double *lmc, int32_t *target_idx, double *edge_dist,
                         double *cost_to_goal, double *radius_used, int32_t *rounds, uint8_t *status) {
  CHECK_CTX(ctx);
  return find_new_target(ctx, "find_new_target", false, pose, nq, r0, r_stride, r_max, robot_radius, 0.0, lmc, target_idx,
                         edge_dist, cost_to_goal, radius_used, rounds, status);
}

int rrtx_find_new_target_dubins(rrtx_ctx *ctx, const double *pose, int nq, const double *r0, int r_stride, double r_max,
                                double robot_radius, double r_min, const double *lmc, int32_t *target_idx,
                                double *edge_dist, double *cost_to_goal, double *radius_used, int32_t *rounds,
                                uint8_t *status) {
  CHECK_CTX(ctx);
  return find_new_target(ctx, "find_new_target_dubins", true, pose, nq, r0, r_stride, r_max, robot_radius, r_min, lmc,
                         target_idx, edge_dist, cost_to_goal, radius_used, rounds, status);
}

}  // extern "C"
