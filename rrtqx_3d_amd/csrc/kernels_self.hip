// kernels_self.hip -- the samples of one extend batch among themselves (rrtx_extend_candidates_self): for every
// sample j the earlier samples i < j of the same batch with KDdist(q_j, q_i) < r, which is what kdFindWithinRange
// adds to j's list when the samples are inserted one after the other (R/kdTree_general.jl:830).  The tree is not read.
//
// Semantics (exact, no tolerance): entry (j, i) exists  <=>  both samples are live (finite, not skipped), i < j and
// s = sq3(q_j, q_i) < thr, thr = sq_first_ge(r) -- the test the range search applies to a non-root node; the key and
// SimpleEdge cost of the entry is sqrt_rn(s).  Rows are in ascending i.
//
// Layout.  A brute-force triangular join in plain launches, no communication between workgroups:
//   self_table_kernel        q -> a table of four doubles per sample (x y z mark; mark != 0: skipped or non-finite, the
//                            sample has no list and is in none), its fp32 shadow relative to the context origin
//                            (x~ y~ z~ |p~|^2; +inf for a marked sample, which the screen then drops) and
//                            C = max |q - origin| over the live samples.  Both sides of every screened pair are
//                            samples, so this C is the bound the proof of the fp32 screen asks for (nn_device.hpp).
//   self_join_kernel<false>  counts every row.
//   excl_scan_kernel         (wave_device.hpp) counts -> offsets, total.
//   self_join_kernel<true>   the same walk again; writes idx, cost and the owner row of every entry.
// The two join passes take the same decisions in the same order: a row is walked by ONE wave, tiles of earlier samples
// in ascending order, and inside a tile the ballot over (u, lane) is ascending in i, so an entry's place is
// offsets[j] + (entries of the row before it) -- no sort, no atomics, nothing depends on which wave finishes first.
//
// Balance.  Row j costs j pair tests.  Rows go in groups of kSelfGroup (kQPI per wave); workgroup w takes group w and
// group G - 1 - w, so every workgroup walks about nq columns in all.  A tile of kChunkF earlier samples is staged in
// LDS once per workgroup and read by its four waves (kScanFU shadows per lane), against which a wave screens kQPI rows
// per iteration with the packed fp32 norm expansion of the range scan (screen8).  A pair is dropped only when the
// screen proves s >= thr; survivors are decided by the unfused fp64 sq3 from the fp64 table.  Nearly every (row, lane)
// has no survivor, so the common path only takes the minimum of the lane's kScanFU screen values and compares once.
#include "nn_device.hpp"

namespace rrtx {
namespace {

constexpr int kSelfThreads = 256;
constexpr int kSelfWaves = kSelfThreads / 64;
constexpr int kSelfGroup = kSelfWaves * kQPI;     // rows per group: kQPI per wave
constexpr int kSelfTile = kChunkF;                // earlier samples per LDS tile: kScanFU per lane

__global__ __launch_bounds__(256) void self_table_kernel(const double *__restrict__ q, int nq,
                                                         const uint8_t *__restrict__ skip, double ox, double oy,
                                                         double oz, double4 *__restrict__ tab,
                                                         float4 *__restrict__ shadow,
                                                         unsigned long long *__restrict__ absmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long m = 0ull;
  if (i < nq) {
    const double a = q[(size_t)i * 3 + 0], b = q[(size_t)i * 3 + 1], c = q[(size_t)i * 3 + 2];
    const bool live = (a - a == 0.0) && (b - b == 0.0) && (c - c == 0.0) && !(skip && skip[i] != 0);
    tab[i] = make_double4(a, b, c, live ? 0.0 : 1.0);
    float4 f = make_float4(0.f, 0.f, 0.f, __builtin_inff());
    if (live) {
      const double sa = a - ox, sb = b - oy, sc = c - oz;
      const float fa = (float)sa, fb = (float)sb, fc = (float)sc;
      const double pp = (double)fa * (double)fa + (double)fb * (double)fb + (double)fc * (double)fc;
      f = make_float4(fa, fb, fc, (float)pp);
      m = max(max((unsigned long long)__double_as_longlong(fabs(sa)), (unsigned long long)__double_as_longlong(fabs(sb))),
              (unsigned long long)__double_as_longlong(fabs(sc)));
    }
    shadow[i] = f;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off);
    m = max(m, o);
  }
  // (a maximum: the value does not depend on the order of the updates)
  if ((threadIdx.x & 63) == 0 && m != 0ull) atomicMax(absmax, m);
}

struct SelfJoin {
  const double4 *tab;
  const float4 *shadow;
  const unsigned long long *absmax;
  int nq;
  double thr, ox, oy, oz;
  int *count;                    // count pass: [nq] row lengths
  const int64_t *offsets;        // fill pass: [nq + 1]
  long long cap;
  int32_t *idx, *owner;
  double *cost;
};

template <bool FILL>
__global__ __launch_bounds__(kSelfThreads) void self_join_kernel(const SelfJoin a) {
  __shared__ float4 tile[2][kSelfTile];
  __shared__ double4 rowd[2 * kSelfGroup];
  __shared__ QRecF3 rowf[2 * kSelfGroup];
  __shared__ int rowj[2 * kSelfGroup];       // the row of a slot, -1: none
  __shared__ int rown[2 * kSelfGroup];       // columns the row is tested against: j, or 0 for a marked sample
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (FILL && a.offsets[a.nq] > a.cap) return;     // the lists do not fit: nothing is written (the caller retries)
  const int G = (a.nq + kSelfGroup - 1) / kSelfGroup;
  const int glo = blockIdx.x, ghi = G - 1 - (int)blockIdx.x;      // glo <= ghi (the grid is (G + 1) / 2)
  if (t < 2 * kSelfGroup) {
    const int half = t / kSelfGroup;
    int j = (half ? ghi : glo) * kSelfGroup + t % kSelfGroup;
    if ((half && ghi == glo) || j >= a.nq) j = -1;
    double4 d = make_double4(0.0, 0.0, 0.0, 1.0);
    if (j >= 0) d = a.tab[j];
    const bool live = j >= 0 && d.w == 0.0;
    QRecF3 f = never_pass_qrecf<3>();
    if (live) {
      QRec3 c;
      c.x = d.x; c.y = d.y; c.z = d.z; c.thr = a.thr;
      f = make_qrecf<3>(c, __longlong_as_double((long long)*a.absmax), a.ox, a.oy, a.oz, 0.0);
    }
    rowd[t] = d; rowf[t] = f; rowj[t] = j; rown[t] = live ? j : 0;
  }
  __syncthreads();
  // per half: the wave's kQPI slots, the columns its longest row needs, and every row's running length
  int hmax[2], cnt[2][kQPI];
  long long base[2][kQPI];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    hmax[h] = 0;
#pragma unroll
    for (int r = 0; r < kQPI; ++r) {
      const int slot = h * kSelfGroup + wave * kQPI + r;
      hmax[h] = max(hmax[h], __builtin_amdgcn_readfirstlane(rown[slot]));
      cnt[h][r] = 0;
      base[h][r] = 0;
      if (FILL && rowj[slot] >= 0) base[h][r] = a.offsets[rowj[slot]];
    }
  }
  const int wmax = max(hmax[0], hmax[1]);
  const int ncols = min(a.nq, (ghi + 1) * kSelfGroup) - 1;        // the workgroup's last row (workgroup-uniform)
  // Two tile buffers, one barrier a tile: a tile is written while the previous one may still be read, and the barrier
  // that publishes it also says that everyone is done with the one before.  The shadows of the NEXT tile are asked for
  // before this one is screened, so their way from memory is hidden behind the screen.
  static_assert(kSelfTile == 2 * kSelfThreads, "two shadows a thread");
  float4 pre0 = make_float4(0.f, 0.f, 0.f, __builtin_inff()), pre1 = pre0;
  if (0 < ncols) {
    if (t < a.nq) pre0 = a.shadow[t];
    if (kSelfThreads + t < a.nq) pre1 = a.shadow[kSelfThreads + t];
  }
  int buf = 0;
  for (int tb = 0; tb < ncols; tb += kSelfTile, buf ^= 1) {
    tile[buf][t] = pre0;
    tile[buf][kSelfThreads + t] = pre1;
    __syncthreads();
    pre0 = make_float4(0.f, 0.f, 0.f, __builtin_inff());
    pre1 = pre0;
    if (tb + kSelfTile < ncols) {
      const int i = tb + kSelfTile + t;
      if (i < a.nq) pre0 = a.shadow[i];
      if (i + kSelfThreads < a.nq) pre1 = a.shadow[i + kSelfThreads];
    }
    if (tb >= wmax) continue;              // (wave-uniform; the barrier above is passed by every wave all the same)
    float x[kScanFU], y[kScanFU], z[kScanFU], pp[kScanFU];
#pragma unroll
    for (int u = 0; u < kScanFU; ++u) {
      const float4 c = tile[buf][u * 64 + lane];
      x[u] = c.x; y[u] = c.y; z[u] = c.z; pp[u] = c.w;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (tb >= hmax[h]) continue;
      // "t > thr'" proves s >= thr, so a row has a survivor among the lane's kScanFU pairs iff !(min t > thr').  (A NaN t
      // needs a coordinate beyond the fp32 range, and then C has set thr' = +inf, which nothing exceeds: every pair
      // survives, whatever the minimum makes of the NaN.)
      bool some[kQPI];
      bool any = false;
#pragma unroll
      for (int r = 0; r < kQPI; ++r) {
        const QRecF3 c = rowf[h * kSelfGroup + wave * kQPI + r];
        float tv[kScanFU];
        screen8<3>(c, x, y, z, nullptr, pp, tv);
        float lo = tv[0];
#pragma unroll
        for (int u = 1; u < kScanFU; ++u) lo = fminf(lo, tv[u]);
        some[r] = !(lo > c.thr);
        any = any || some[r];
      }
      if (__ballot(any) == 0ull) continue;
      // rare: some pair of these rows survived the screen -> the exact test decides
#pragma unroll
      for (int r = 0; r < kQPI; ++r) {
        if (__ballot(some[r]) == 0ull) continue;
        const int slot = h * kSelfGroup + wave * kQPI + r;
        const int jn = __builtin_amdgcn_readfirstlane(rown[slot]);
        const double4 rd = rowd[slot];
        const QRecF3 c = rowf[slot];
        float tv[kScanFU];
        screen8<3>(c, x, y, z, nullptr, pp, tv);
#pragma unroll
        for (int u = 0; u < kScanFU; ++u) {
          const bool surv = !(tv[u] > c.thr);
          if (__ballot(surv) == 0ull) continue;
          const int i = tb + u * 64 + lane;
          double s = 0.0;
          bool hit = false;
          if (surv && i < jn) {                          // i < j <= nq - 1: inside the table
            const double4 ci = a.tab[i];
            s = sq3(rd.x, rd.y, rd.z, ci.x, ci.y, ci.z);
            hit = ci.w == 0.0 && s < a.thr;
          }
          const unsigned long long b = __ballot(hit);
          if (FILL && hit) {
            const long long pos = base[h][r] + cnt[h][r] + __popcll(b & lanes_below(lane));
            if (pos < a.cap) {
              a.idx[pos] = i;
              a.cost[pos] = sqrt_rn(s);
              a.owner[pos] = rowj[slot];
            }
          }
          cnt[h][r] += __popcll(b);
        }
      }
    }
  }
  if (!FILL && lane == 0) {
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int r = 0; r < kQPI; ++r) {
        const int j = rowj[h * kSelfGroup + wave * kQPI + r];
        if (j >= 0) a.count[j] = cnt[h][r];
      }
  }
}

}  // namespace

int launch_self_join(rrtx_ctx *ctx, const double *q_dev, int nq, double r, const uint8_t *skip_dev, int64_t *offsets_dev,
                     int32_t *idx_dev, double *cost_dev, int32_t *owner_dev, int64_t cap, int64_t *needed_dev,
                     const double **table_out) {
  if (nq <= 0) return RRTX_OK;
  // ws_self: table (32 B a sample), shadow (16 B), row counts, C
  const size_t n = (size_t)nq;
  const size_t off_shadow = sizeof(double4) * n, off_count = off_shadow + sizeof(float4) * n;
  const size_t off_max = (off_count + sizeof(int) * (n + 1) + 7) & ~(size_t)7;
  RRTX_HIP(ctx, ctx->ws_self.ensure(off_max + sizeof(unsigned long long)));
  char *ws = ctx->ws_self.as<char>();
  double4 *tab = reinterpret_cast<double4 *>(ws);
  float4 *shadow = reinterpret_cast<float4 *>(ws + off_shadow);
  int *count = reinterpret_cast<int *>(ws + off_count);
  unsigned long long *absmax = reinterpret_cast<unsigned long long *>(ws + off_max);
  RRTX_HIP(ctx, hipMemsetAsync(absmax, 0, sizeof(unsigned long long), ctx->stream));
  SelfJoin a;
  a.tab = tab; a.shadow = shadow; a.absmax = absmax; a.nq = nq;
  a.thr = thr_first_ge(r);
  a.ox = ctx->origin[0]; a.oy = ctx->origin[1]; a.oz = ctx->origin[2];
  a.count = count; a.offsets = offsets_dev; a.cap = (long long)cap;
  a.idx = idx_dev; a.owner = owner_dev; a.cost = cost_dev;
  const int G = (nq + kSelfGroup - 1) / kSelfGroup;
  const dim3 grid((unsigned)((G + 1) / 2));
  span_begin(ctx, KF_NN_SCAN);
  hipLaunchKernelGGL(self_table_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, q_dev, nq, skip_dev,
                     a.ox, a.oy, a.oz, tab, shadow, absmax);
  hipLaunchKernelGGL(self_join_kernel<false>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  launch_excl_scan<int64_t>(ctx->stream, count, offsets_dev, nq, needed_dev);
  if (cap > 0) hipLaunchKernelGGL(self_join_kernel<true>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  if (table_out) *table_out = reinterpret_cast<const double *>(tab);
  return RRTX_OK;
}

}  // namespace rrtx
