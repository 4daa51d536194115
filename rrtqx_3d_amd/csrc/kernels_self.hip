// kernels_self.hip -- the samples of one extend batch among themselves (rrtx_extend_candidates_self): for every
// sample j the earlier samples i < j of the same batch with KDdist(q_j, q_i) < r, which is what kdFindWithinRange
// adds to j's list when the samples are inserted one after the other (R/kdTree_general.jl:830).  The tree is not read.
// The [x y t theta] form with wrapped dimensions (rrtx_extend_candidates_self_dubins) is the second half of the file.
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

// ---- the same join in [x y t theta] with wrapped dimensions (rrtx_extend_candidates_self_dubins) -----------------
// Sibling kernels, so the 3-D instantiations above keep their machine code.  The row sample j is the query: it has
// 2^w copies by nn_pack's rule (slot 0 the sample itself, slot k shifts the wrapped dimensions whose bit is set in k,
// the LAST wrapped dimension the least significant bit; a ghost is skipped when sq4(closest, ghost) >= thr_gt).  The
// column sample i plays the node and is taken as it is.  Entry (j, i) exists  <=>  both are live, i < j and some
// non-skipped slot k has s_k = sq4(copy_k(q_j), q_i) < thr; the key is sqrt_rn(s_k) of the LOWEST such k
// (addToRangeList keeps the first discovery: seen_by_earlier_slot in the tree search).
//   self_table4_kernel       q -> the four coordinate columns the Dubins edge source reads, a mark byte per sample, the
//                            fp32 shadow (x~ y~ z~ w~ and |p~|^2 apart; +inf for a marked sample) and
//                            C = max |g - origin| over every non-skipped copy g of every live sample: the proof of the
//                            screen needs both sides of a screened pair inside C, and a ghost lies up to a period
//                            outside the samples' extent.
//   self_join4_kernel<FILL>  the walk of self_join_kernel; a (row, lane) goes to the rare path when the screen of ANY
//                            copy of the row fails to prove s >= thr for one of the lane's columns, and there the exact
//                            sq4 decides, slots ascending, the first hit giving the key.
struct SelfWrap {
  int n_wraps;
  int wd[3];
  double wp[3];
  double thr_gt;
};

// copy k of the sample p (nn_pack_kernel, the "for k < n_slots" loop); false: the ghost iterator skips it
__device__ __forceinline__ bool self_copy(const SelfWrap &wr, const double *p, int k, double *g) {
  double c[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) { g[d] = p[d]; c[d] = p[d]; }
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    if (w >= wr.n_wraps || !((k >> (wr.n_wraps - 1 - w)) & 1)) continue;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (wr.wd[w] != d) continue;
      double dim_val = p[d], dim_closest = 0.0;
      if (p[d] < wr.wp[w] / 2.0) { dim_val += wr.wp[w]; dim_closest += wr.wp[w]; }
      else { dim_val -= wr.wp[w]; }
      g[d] = dim_val;
      c[d] = dim_closest;
    }
  }
  if (k == 0) return true;
  return !(sq4(c[0], c[1], c[2], c[3], g[0], g[1], g[2], g[3]) >= wr.thr_gt);
}

constexpr int kSelfSlots = 8;                     // copies of a sample: 2^w, w <= 3

__global__ __launch_bounds__(256) void self_table4_kernel(const double *__restrict__ q, int nq,
                                                          const uint8_t *__restrict__ skip, const SelfWrap wr, double ox,
                                                          double oy, double oz, double ow, double *__restrict__ nx,
                                                          double *__restrict__ ny, double *__restrict__ nz,
                                                          double *__restrict__ nw, uint8_t *__restrict__ mark,
                                                          float4 *__restrict__ shadow, float *__restrict__ spp,
                                                          unsigned long long *__restrict__ absmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned long long m = 0ull;
  if (i < nq) {
    double p[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) p[d] = q[(size_t)i * 4 + d];
    const bool live = (p[0] - p[0] == 0.0) && (p[1] - p[1] == 0.0) && (p[2] - p[2] == 0.0) && (p[3] - p[3] == 0.0) &&
                      !(skip && skip[i] != 0);
    nx[i] = p[0]; ny[i] = p[1]; nz[i] = p[2]; nw[i] = p[3];
    mark[i] = live ? 0 : 1;
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    float fpp = __builtin_inff();
    if (live) {
      const double o[4] = {ox, oy, oz, ow};
      const float fa = (float)(p[0] - ox), fb = (float)(p[1] - oy), fc = (float)(p[2] - oz), fd = (float)(p[3] - ow);
      const double pp = (double)fa * (double)fa + (double)fb * (double)fb + (double)fc * (double)fc + (double)fd * (double)fd;
      f = make_float4(fa, fb, fc, fd);
      fpp = (float)pp;
      const int n_slots = 1 << wr.n_wraps;
      for (int k = 0; k < n_slots; ++k) {
        double g[4];
        if (!self_copy(wr, p, k, g)) continue;
#pragma unroll
        for (int d = 0; d < 4; ++d) m = max(m, (unsigned long long)__double_as_longlong(fabs(g[d] - o[d])));
      }
    }
    shadow[i] = f;
    spp[i] = fpp;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(m, off);
    m = max(m, o);
  }
  // (a maximum: the value does not depend on the order of the updates)
  if ((threadIdx.x & 63) == 0 && m != 0ull) atomicMax(absmax, m);
}

struct SelfJoin4 {
  const double *nx, *ny, *nz, *nw;
  const uint8_t *mark;
  const float4 *shadow;
  const float *spp;
  const unsigned long long *absmax;
  int nq;
  double thr, ox, oy, oz, ow;
  SelfWrap wr;
  int *count;                    // count pass: [nq] row lengths
  const int64_t *offsets;        // fill pass: [nq + 1]
  long long cap;
  int32_t *idx, *owner;
  double *key;
};

template <bool FILL>
__global__ __launch_bounds__(kSelfThreads) void self_join4_kernel(const SelfJoin4 a) {
  __shared__ float4 tile[2][kSelfTile];
  __shared__ float tilep[2][kSelfTile];
  __shared__ double4 rowg[2 * kSelfGroup][kSelfSlots];     // the copies of a row's sample
  __shared__ QRecF4 rowf[2 * kSelfGroup][kSelfSlots];      // ... and their screen records (never_pass: no such copy)
  __shared__ int rowj[2 * kSelfGroup];       // the row of a slot, -1: none
  __shared__ int rown[2 * kSelfGroup];       // columns the row is tested against: j, or 0 for a marked sample
  __shared__ int rowv[2 * kSelfGroup];       // bit k: copy k exists (live sample, k < 2^w, not skipped by the ghost rule)
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  if (FILL && a.offsets[a.nq] > a.cap) return;     // the lists do not fit: nothing is written (the caller retries)
  const int G = (a.nq + kSelfGroup - 1) / kSelfGroup;
  const int glo = blockIdx.x, ghi = G - 1 - (int)blockIdx.x;      // glo <= ghi (the grid is (G + 1) / 2)
  const int ns = 1 << a.wr.n_wraps;
  static_assert(2 * kSelfGroup * kSelfSlots == kSelfThreads, "a thread per (row, copy)");
  {
    const int slot = t / kSelfSlots, k = t % kSelfSlots;
    const int half = slot / kSelfGroup;
    int j = (half ? ghi : glo) * kSelfGroup + slot % kSelfGroup;
    if ((half && ghi == glo) || j >= a.nq) j = -1;
    const bool live = j >= 0 && a.mark[j] == 0;
    double4 g4 = make_double4(0.0, 0.0, 0.0, 0.0);
    QRecF4 f = never_pass_qrecf<4>();
    bool valid = false;
    if (live && k < ns) {
      const double p[4] = {a.nx[j], a.ny[j], a.nz[j], a.nw[j]};
      double g[4];
      valid = self_copy(a.wr, p, k, g);
      g4 = make_double4(g[0], g[1], g[2], g[3]);
      if (valid) {
        QRec4 c;
        c.x = g[0]; c.y = g[1]; c.z = g[2]; c.w = g[3]; c.thr = a.thr; c.pad0 = 0.0; c.pad1 = 0.0; c.pad2 = 0.0;
        f = make_qrecf<4>(c, __longlong_as_double((long long)*a.absmax), a.ox, a.oy, a.oz, a.ow);
      }
    }
    rowg[slot][k] = g4; rowf[slot][k] = f;
    const unsigned long long vb = __ballot(valid);
    if (k == 0) {
      rowj[slot] = j; rown[slot] = live ? j : 0;
      rowv[slot] = (int)((vb >> (lane & ~(kSelfSlots - 1))) & (unsigned long long)((1 << kSelfSlots) - 1));
    }
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
  // (two tile buffers, one barrier a tile, the next tile's shadows asked for before this one is screened: as above)
  const float4 none4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 pre0 = none4, pre1 = none4;
  float prep0 = __builtin_inff(), prep1 = prep0;
  if (0 < ncols) {
    if (t < a.nq) { pre0 = a.shadow[t]; prep0 = a.spp[t]; }
    if (kSelfThreads + t < a.nq) { pre1 = a.shadow[kSelfThreads + t]; prep1 = a.spp[kSelfThreads + t]; }
  }
  int buf = 0;
  for (int tb = 0; tb < ncols; tb += kSelfTile, buf ^= 1) {
    tile[buf][t] = pre0; tilep[buf][t] = prep0;
    tile[buf][kSelfThreads + t] = pre1; tilep[buf][kSelfThreads + t] = prep1;
    __syncthreads();
    pre0 = none4; pre1 = none4;
    prep0 = __builtin_inff(); prep1 = prep0;
    if (tb + kSelfTile < ncols) {
      const int i = tb + kSelfTile + t;
      if (i < a.nq) { pre0 = a.shadow[i]; prep0 = a.spp[i]; }
      if (i + kSelfThreads < a.nq) { pre1 = a.shadow[i + kSelfThreads]; prep1 = a.spp[i + kSelfThreads]; }
    }
    if (tb >= wmax) continue;              // (wave-uniform; the barrier above is passed by every wave all the same)
    float x[kScanFU], y[kScanFU], z[kScanFU], w[kScanFU], pp[kScanFU];
#pragma unroll
    for (int u = 0; u < kScanFU; ++u) {
      const float4 c = tile[buf][u * 64 + lane];
      x[u] = c.x; y[u] = c.y; z[u] = c.z; w[u] = c.w; pp[u] = tilep[buf][u * 64 + lane];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (tb >= hmax[h]) continue;
      // a row has a survivor among the lane's kScanFU pairs iff for some copy !(min t > thr') (a NaN t: as above)
      bool some[kQPI];
      bool any = false;
#pragma unroll
      for (int r = 0; r < kQPI; ++r) {
        some[r] = false;
        for (int k = 0; k < ns; ++k) {
          const QRecF4 c = rowf[h * kSelfGroup + wave * kQPI + r][k];
          float tv[kScanFU];
          screen8<4>(c, x, y, z, w, pp, tv);
          float lo = tv[0];
#pragma unroll
          for (int u = 1; u < kScanFU; ++u) lo = fminf(lo, tv[u]);
          some[r] = some[r] || !(lo > c.thr);
        }
        any = any || some[r];
      }
      if (__ballot(any) == 0ull) continue;
      // rare: some pair of these rows survived the screen of some copy -> the exact test decides
#pragma unroll
      for (int r = 0; r < kQPI; ++r) {
        if (__ballot(some[r]) == 0ull) continue;
        const int slot = h * kSelfGroup + wave * kQPI + r;
        const int jn = __builtin_amdgcn_readfirstlane(rown[slot]);
        const int vmask = __builtin_amdgcn_readfirstlane(rowv[slot]);
        unsigned sm = 0u;                    // bit u: the lane's column u survived the screen of some copy
        for (int k = 0; k < ns; ++k) {
          const QRecF4 c = rowf[slot][k];
          float tv[kScanFU];
          screen8<4>(c, x, y, z, w, pp, tv);
#pragma unroll
          for (int u = 0; u < kScanFU; ++u) sm |= !(tv[u] > c.thr) ? (1u << u) : 0u;
        }
#pragma unroll
        for (int u = 0; u < kScanFU; ++u) {
          const bool surv = ((sm >> u) & 1u) != 0u;
          if (__ballot(surv) == 0ull) continue;
          const int i = tb + u * 64 + lane;
          double s = 0.0;
          bool hit = false;
          if (surv && i < jn && a.mark[i] == 0) {        // i < j <= nq - 1: inside the table
            const double cx = a.nx[i], cy = a.ny[i], cz = a.nz[i], cw = a.nw[i];
            for (int k = 0; k < ns && !hit; ++k) {       // slots ascending: the first hit gives the key
              if (!((vmask >> k) & 1)) continue;
              const double4 g = rowg[slot][k];
              s = sq4(g.x, g.y, g.z, g.w, cx, cy, cz, cw);
              hit = s < a.thr;
            }
          }
          const unsigned long long b = __ballot(hit);
          if (FILL && hit) {
            const long long pos = base[h][r] + cnt[h][r] + __popcll(b & lanes_below(lane));
            if (pos < a.cap) {
              a.idx[pos] = i;
              a.key[pos] = sqrt_rn(s);
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

int launch_self_join_dubins(rrtx_ctx *ctx, const double *q_dev, int nq, double r, const uint8_t *skip_dev,
                            int64_t *offsets_dev, int32_t *idx_dev, double *key_dev, int32_t *owner_dev, int64_t cap,
                            int64_t *needed_dev, const double **columns_out) {
  if (nq <= 0) return RRTX_OK;
  // ws_self: four coordinate columns (32 B a sample), shadow (16 B), its norms (4 B), row counts, C, marks
  const size_t n = (size_t)nq;
  const size_t off_shadow = sizeof(double) * 4 * n, off_spp = off_shadow + sizeof(float4) * n;
  const size_t off_count = off_spp + sizeof(float) * n;
  const size_t off_max = (off_count + sizeof(int) * (n + 1) + 7) & ~(size_t)7;
  const size_t off_mark = off_max + sizeof(unsigned long long);
  RRTX_HIP(ctx, ctx->ws_self.ensure(off_mark + n));
  char *ws = ctx->ws_self.as<char>();
  double *col = reinterpret_cast<double *>(ws);
  unsigned long long *absmax = reinterpret_cast<unsigned long long *>(ws + off_max);
  RRTX_HIP(ctx, hipMemsetAsync(absmax, 0, sizeof(unsigned long long), ctx->stream));
  SelfJoin4 a;
  a.nx = col; a.ny = col + n; a.nz = col + 2 * n; a.nw = col + 3 * n;
  a.mark = reinterpret_cast<const uint8_t *>(ws + off_mark);
  a.shadow = reinterpret_cast<const float4 *>(ws + off_shadow);
  a.spp = reinterpret_cast<const float *>(ws + off_spp);
  a.absmax = absmax; a.nq = nq;
  a.thr = thr_first_ge(r);
  a.ox = ctx->origin[0]; a.oy = ctx->origin[1]; a.oz = ctx->origin[2]; a.ow = ctx->origin[3];
  a.wr.n_wraps = ctx->n_wraps;
  for (int w = 0; w < 3; ++w) { a.wr.wd[w] = ctx->wrap_dim[w]; a.wr.wp[w] = ctx->wrap_period[w]; }
  a.wr.thr_gt = thr_first_gt(r);
  a.count = reinterpret_cast<int *>(ws + off_count); a.offsets = offsets_dev; a.cap = (long long)cap;
  a.idx = idx_dev; a.owner = owner_dev; a.key = key_dev;
  const int G = (nq + kSelfGroup - 1) / kSelfGroup;
  const dim3 grid((unsigned)((G + 1) / 2));
  span_begin(ctx, KF_NN_SCAN);
  hipLaunchKernelGGL(self_table4_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, q_dev, nq, skip_dev,
                     a.wr, a.ox, a.oy, a.oz, a.ow, col, col + n, col + 2 * n, col + 3 * n,
                     reinterpret_cast<uint8_t *>(ws + off_mark), reinterpret_cast<float4 *>(ws + off_shadow),
                     reinterpret_cast<float *>(ws + off_spp), absmax);
  hipLaunchKernelGGL(self_join4_kernel<false>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  launch_excl_scan<int64_t>(ctx->stream, a.count, offsets_dev, nq, needed_dev);
  if (cap > 0) hipLaunchKernelGGL(self_join4_kernel<true>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  if (columns_out) *columns_out = col;
  return RRTX_OK;
}

}  // namespace rrtx
