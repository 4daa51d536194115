// kernels_self.hip -- the samples of one extend batch among themselves (rrtx_extend_candidates_self): for every
// sample j the earlier samples i < j of the same batch with KDdist(q_j, q_i) < r, which is what kdFindWithinRange
// adds to j's list when the samples are inserted one after the other (R/kdTree_general.jl:830).  The tree is not read.
// The [x y t theta] form with wrapped dimensions (rrtx_extend_candidates_self_dubins) is the second half of the file,
// the k nearest earlier samples for the closestNode rule (rrtx_extend_closest_self) the third.
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
#include "block_layout.hpp"

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

// ---- the k nearest earlier samples of a batch (rrtx_extend_closest_self) ------------------------------------------
// For a wanted live sample j the first k of the live samples i < j, ordered by (s, i), s = sq3(q_j, q_i) finite: what the
// closestNode rule of findBestParent needs when the ball of j is empty and kdFindNearest may answer with a sample of the
// same batch.  Fixed-width rows, so one pass: no count / fill pair.
//   self_table_kernel     as above: table, shadows, C.
//   closest_fill_kernel   every slot of every row to "none" (idx -1, cost +Inf, flags 0, count 0), the owner row of
//                         every slot for the edge kernels, the tree column's flags to 0.
//   closest_plan_kernel   ONE workgroup: the wanted live rows, ascending, to a compact list, so that the row kernel's work
//                         follows their number; the tree column's node index of a filled row (-1 otherwise); and the
//                         number of slots / rows the edge kernels have to look at (up to the last filled row).
//   closest_rows_kernel   a wave owns a row of the compact list and walks the earlier samples in ascending tiles staged
//                         in LDS, as the join does.  It keeps the row's best k pairs (s, i) sorted, pair l in lane l;
//                         tau is the k-th s, +Inf until the row is full.  The fp32 screen is the join's with thr = tau:
//                         it drops a pair only when it proves s >= tau, which on a full row loses against every pair
//                         held (columns arrive in ascending i, so a later index loses a tie).  Survivors are decided by
//                         the unfused fp64 sq3 and inserted one at a time in ascending i (a v_readlane and a DPP wave
//                         shift, no LDS crossbar); tau follows every insertion, the screen record once a tile.  The
//                         groups of rows are dealt heaviest first.
// A row's result is a function of its columns in ascending order alone: nothing depends on the launch geometry or on
// which wave finishes first.
// A row is a chain of dependent steps -- about 8 (1 + ln(j / 512)) + 8 survivors after the first tile, each a trip to the
// fp64 table, and as many insertions -- so the kernel is bound by that chain's latency times the rows a wave owns, not
// by the screen: at B = 16 384, k = 8, all rows wanted, it took 204 us with 4 rows a wave and 127 us with one
// (DESIGN.md 4.19).
constexpr int kClosestRows = 1;                               // rows a wave owns
constexpr int kClosestGroup = kSelfWaves * kClosestRows;      // rows a workgroup owns
constexpr int kPlanThreads = 1024;

__global__ __launch_bounds__(256) void closest_fill_kernel(int nq, int k, int32_t *__restrict__ idx,
                                                           double *__restrict__ cost, uint8_t *__restrict__ hit_out,
                                                           uint8_t *__restrict__ hit_in, int32_t *__restrict__ count,
                                                           int32_t *__restrict__ owner, int32_t *__restrict__ row_owner,
                                                           uint8_t *__restrict__ tree_hit_out,
                                                           uint8_t *__restrict__ tree_hit_in) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)nq * k) return;
  idx[e] = -1;
  cost[e] = __builtin_inf();
  hit_out[e] = 0;
  hit_in[e] = 0;
  owner[e] = (int32_t)(e / k);
  if (e < nq) {
    count[e] = 0;
    row_owner[e] = (int32_t)e;
    if (tree_hit_out) { tree_hit_out[e] = 0; tree_hit_in[e] = 0; }
  }
}

struct ClosestPlan {
  const double4 *tab;
  const uint8_t *want;           // [nq] or null: every live row
  const int32_t *tree_idx;       // [nq] or null
  int nq, k;
  int *rows;                     // [nq] the filled rows, ascending
  int *n_rows;                   // their number
  int32_t *tree_near;            // [nq] tree_idx of a filled row, -1 otherwise (null with tree_idx)
  int64_t *slots_end;            // (last filled row + 1) * k: the "offsets[nq]" of the slot entries
  int64_t *rows_end;             // last filled row + 1: the same for the tree column
};

__global__ __launch_bounds__(kPlanThreads) void closest_plan_kernel(const ClosestPlan a) {
  __shared__ int wcnt[2][kPlanThreads / 64], wlast[2][kPlanThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int base = 0, last = -1, flip = 0;
  for (int j0 = 0; j0 < a.nq; j0 += kPlanThreads, flip ^= 1) {
    const int j = j0 + t;
    const bool fill = j < a.nq && a.tab[j].w == 0.0 && (!a.want || a.want[j] != 0);
    const unsigned long long votes = __ballot(fill);
    if (lane == 0) {
      wcnt[flip][wave] = __popcll(votes);
      wlast[flip][wave] = votes != 0ull ? j0 + wave * 64 + 63 - __clzll((long long)votes) : -1;
    }
    __syncthreads();                       // (two sets of counts: the next round's writes cannot overtake this round's reads)
    int before = 0, total = 0;
    for (int w = 0; w < kPlanThreads / 64; ++w) {
      const int c = wcnt[flip][w];
      if (w < wave) before += c;
      total += c;
      last = max(last, wlast[flip][w]);
    }
    if (fill) a.rows[base + before + __popcll(votes & lanes_below(lane))] = j;
    if (j < a.nq && a.tree_near) a.tree_near[j] = fill ? a.tree_idx[j] : -1;
    base += total;
  }
  if (t == 0) {
    *a.n_rows = base;
    *a.slots_end = (int64_t)(last + 1) * a.k;
    *a.rows_end = (int64_t)(last + 1);
  }
}

// lane l's value to every lane (l wave-uniform), and every lane's value to the lane above it (lane 0 keeps its own):
// v_readlane_b32 and a DPP wave shift, no LDS crossbar
__device__ __forceinline__ int wave_read(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ double wave_read(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ int wave_shift_up(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x138, 0xf, 0xf, false); }
__device__ __forceinline__ double wave_shift_up(double v) {
  return __hiloint2double(wave_shift_up(__double2hiint(v)), wave_shift_up(__double2loint(v)));
}

struct ClosestRows {
  const double4 *tab;
  const float4 *shadow;
  const unsigned long long *absmax;
  const int *rows, *n_rows;
  int nq, k;
  double ox, oy, oz;
  int32_t *idx, *count;
  double *cost;
};

__global__ __launch_bounds__(kSelfThreads) void closest_rows_kernel(const ClosestRows a) {
  __shared__ float4 tile[2][kSelfTile];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nr = min(max(*a.n_rows, 0), a.nq);
  const int G = (nr + kClosestGroup - 1) / kClosestGroup;
  if ((int)blockIdx.x >= G) return;                         // (workgroup-uniform)
  const int g = G - 1 - (int)blockIdx.x;                    // heaviest group first
  const double C = __longlong_as_double((long long)*a.absmax);
  // the wave's rows: sample, columns, the pairs held (pair l in lane l), tau and the screen record for it
  int rj[kClosestRows], cnt[kClosestRows], bi[kClosestRows];
  double px[kClosestRows], py[kClosestRows], pz[kClosestRows], tau[kClosestRows], tauf[kClosestRows], bs[kClosestRows];
  const unsigned long long kmask = lanes_below(a.k);        // (k <= 32)
  QRecF3 rf[kClosestRows];
  int wmax = 0;
#pragma unroll
  for (int r = 0; r < kClosestRows; ++r) {
    const int c = g * kClosestGroup + wave * kClosestRows + r;
    int j = c < nr ? a.rows[c] : -1;
    if ((unsigned)j >= (unsigned)a.nq) j = -1;
    j = __builtin_amdgcn_readfirstlane(j);
    double4 d = make_double4(0.0, 0.0, 0.0, 1.0);
    if (j >= 0) d = a.tab[j];
    rj[r] = j; cnt[r] = 0; bi[r] = -1;
    px[r] = d.x; py[r] = d.y; pz[r] = d.z;
    tau[r] = __builtin_inf(); tauf[r] = tau[r]; bs[r] = __builtin_inf();
    QRec3 c3;
    c3.x = d.x; c3.y = d.y; c3.z = d.z; c3.thr = tau[r];
    rf[r] = j >= 0 ? make_qrecf<3>(c3, C, a.ox, a.oy, a.oz, 0.0) : never_pass_qrecf<3>();
    wmax = max(wmax, j);
  }
  // the workgroup's last row is the last of its group (the list is ascending): columns 0 .. ncols - 1
  int ncols = a.rows[min(nr, (g + 1) * kClosestGroup) - 1];
  ncols = min(max(ncols, 0), a.nq - 1);
  // (two tile buffers, one barrier a tile, the next tile's shadows asked for before this one is screened: as in the join)
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
    for (int r = 0; r < kClosestRows; ++r) {
      if (tb >= rj[r]) continue;
      // "t > thr'" proves s >= tau (thr' = +Inf while the row is not full, and with a non-finite or huge C: nothing is
      // dropped then); the values do not depend on tau, only the comparison does
      float tv[kScanFU];
      screen8<3>(rf[r], x, y, z, nullptr, pp, tv);
      float lo = tv[0];
#pragma unroll
      for (int u = 1; u < kScanFU; ++u) lo = fminf(lo, tv[u]);
      if (__ballot(!(lo > rf[r].thr)) == 0ull) continue;
#pragma unroll
      for (int u = 0; u < kScanFU; ++u) {
        const bool surv = !(tv[u] > rf[r].thr);
        if (__ballot(surv) == 0ull) continue;
        const int i = tb + u * 64 + lane;
        double s = __builtin_inf();
        bool hit = false;
        if (surv && i < rj[r]) {                           // i < j <= nq - 1: inside the table
          const double4 ci = a.tab[i];
          if (ci.w == 0.0) {
            s = sq3(px[r], py[r], pz[r], ci.x, ci.y, ci.z);
            hit = s < tau[r];                              // (a non-finite s is in no row)
          }
        }
        // the lanes' pairs go in one at a time, ascending in i; each insertion may lower tau and drop the rest
        unsigned long long b = __ballot(hit);
        while (b != 0ull) {
          const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)b) - 1);
          const double ns = wave_read(s, l);
          const int ni = tb + u * 64 + l;
          // the pairs held have lower indices, so the new one goes behind every pair with the same s (lanes k and up
          // hold what fell off the row: not counted, never read)
          const int pos = __popcll(__ballot(bs[r] <= ns) & kmask);
          const double us = wave_shift_up(bs[r]);
          const int ui = wave_shift_up(bi[r]);
          if (lane > pos) { bs[r] = us; bi[r] = ui; }
          else if (lane == pos) { bs[r] = ns; bi[r] = ni; }
          cnt[r] = min(cnt[r] + 1, a.k);
          if (cnt[r] == a.k) tau[r] = wave_read(bs[r], a.k - 1);
          hit = hit && lane != l && s < tau[r];
          b = __ballot(hit);
        }
      }
      // the screen record follows tau once a tile: a stale (higher) tau only lets more pairs through to the exact test
      if (tau[r] != tauf[r]) {
        tauf[r] = tau[r];
        QRec3 c3;
        c3.x = px[r]; c3.y = py[r]; c3.z = pz[r]; c3.thr = tau[r];
        rf[r] = make_qrecf<3>(c3, C, a.ox, a.oy, a.oz, 0.0);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kClosestRows; ++r) {
    if (rj[r] < 0) continue;
    if (lane < cnt[r]) {
      a.idx[(size_t)rj[r] * a.k + lane] = bi[r];
      a.cost[(size_t)rj[r] * a.k + lane] = sqrt_rn(bs[r]);
    }
    if (lane == 0) a.count[rj[r]] = cnt[r];
  }
}

// ---- the same rows in [x y t theta] with wrapped dimensions (rrtx_extend_closest_self_dubins) ---------------------
// Sibling kernels once more, so everything above keeps its machine code.  The row sample j is the query with its 2^w
// copies (self_copy's slots; NONE is skipped: there is no radius to skip by), the column sample i is taken as it is, and
//   s(j, i) = min over the slots of sq4(copy_slot(q_j), q_i),
// the distance kdFindNearest settles on once it has handed out its ghosts.  A row holds the first k of the live i < j
// with finite s, ordered by (s, i); the key is sqrt_rn(s).
//   self_table4_kernel     as above with thr_gt = +Inf: no copy is left out of C, which the screen's proof asks for.
//   closest_fill4_kernel   every slot to "none" (idx -1, key and both costs +Inf, words and flags 0, count 0), the owner
//                          row of every slot, the tree column's defaults.
//   closest_plan4_kernel   closest_plan_kernel with the table's mark byte as the live mark.
//   closest_rows4_kernel   closest_rows_kernel's walk.  The row's copies and their screen records are wave-uniform: a
//                          small LDS block per wave, written by the wave's first lanes and read as a broadcast.  The slot
//                          count is a loop bound (1, 2, 4, 8), one kernel for every w.  A column goes to the exact test
//                          unless EVERY copy's screen proves s_slot >= tau; there s is the minimum over all slots from
//                          the fp64 columns and the pair is taken iff s < tau.
__global__ __launch_bounds__(256) void closest_fill4_kernel(int nq, int k, int32_t *__restrict__ idx, double *__restrict__ key,
                                                            double *__restrict__ cost_out, double *__restrict__ cost_in,
                                                            uint8_t *__restrict__ word_out, uint8_t *__restrict__ word_in,
                                                            uint8_t *__restrict__ hit_out, uint8_t *__restrict__ hit_in,
                                                            int32_t *__restrict__ count, int32_t *__restrict__ owner,
                                                            int32_t *__restrict__ row_owner,
                                                            double *__restrict__ tree_cost_out,
                                                            double *__restrict__ tree_cost_in,
                                                            uint8_t *__restrict__ tree_word_out,
                                                            uint8_t *__restrict__ tree_word_in,
                                                            uint8_t *__restrict__ tree_hit_out,
                                                            uint8_t *__restrict__ tree_hit_in) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)nq * k) return;
  idx[e] = -1;
  key[e] = __builtin_inf();
  cost_out[e] = __builtin_inf();
  cost_in[e] = __builtin_inf();
  if (word_out) { word_out[3 * e] = 0; word_out[3 * e + 1] = 0; word_out[3 * e + 2] = 0; }
  if (word_in) { word_in[3 * e] = 0; word_in[3 * e + 1] = 0; word_in[3 * e + 2] = 0; }
  hit_out[e] = 0;
  hit_in[e] = 0;
  owner[e] = (int32_t)(e / k);
  if (e < nq) {
    count[e] = 0;
    row_owner[e] = (int32_t)e;
    if (tree_hit_out) {
      tree_cost_out[e] = __builtin_inf(); tree_cost_in[e] = __builtin_inf();
      tree_hit_out[e] = 0; tree_hit_in[e] = 0;
      if (tree_word_out) { tree_word_out[3 * e] = 0; tree_word_out[3 * e + 1] = 0; tree_word_out[3 * e + 2] = 0; }
      if (tree_word_in) { tree_word_in[3 * e] = 0; tree_word_in[3 * e + 1] = 0; tree_word_in[3 * e + 2] = 0; }
    }
  }
}

struct ClosestPlan4 {
  const uint8_t *mark;           // [nq] the table's mark byte: != 0: skipped or non-finite
  const uint8_t *want;           // [nq] or null: every live row
  const int32_t *tree_idx;       // [nq] or null
  int nq, k;
  int *rows;                     // [nq] the filled rows, ascending
  int *n_rows;                   // their number
  int32_t *tree_near;            // [nq] tree_idx of a filled row, -1 otherwise (null with tree_idx)
  int64_t *slots_end;            // (last filled row + 1) * k: the "offsets[nq]" of the slot entries
  int64_t *rows_end;             // last filled row + 1: the same for the tree column
};

__global__ __launch_bounds__(kPlanThreads) void closest_plan4_kernel(const ClosestPlan4 a) {
  __shared__ int wcnt[2][kPlanThreads / 64], wlast[2][kPlanThreads / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int base = 0, last = -1, flip = 0;
  for (int j0 = 0; j0 < a.nq; j0 += kPlanThreads, flip ^= 1) {
    const int j = j0 + t;
    const bool fill = j < a.nq && a.mark[j] == 0 && (!a.want || a.want[j] != 0);
    const unsigned long long votes = __ballot(fill);
    if (lane == 0) {
      wcnt[flip][wave] = __popcll(votes);
      wlast[flip][wave] = votes != 0ull ? j0 + wave * 64 + 63 - __clzll((long long)votes) : -1;
    }
    __syncthreads();                       // (two sets of counts, as in closest_plan_kernel)
    int before = 0, total = 0;
    for (int w = 0; w < kPlanThreads / 64; ++w) {
      const int c = wcnt[flip][w];
      if (w < wave) before += c;
      total += c;
      last = max(last, wlast[flip][w]);
    }
    if (fill) a.rows[base + before + __popcll(votes & lanes_below(lane))] = j;
    if (j < a.nq && a.tree_near) a.tree_near[j] = fill ? a.tree_idx[j] : -1;
    base += total;
  }
  if (t == 0) {
    *a.n_rows = base;
    *a.slots_end = (int64_t)(last + 1) * a.k;
    *a.rows_end = (int64_t)(last + 1);
  }
}

struct ClosestRows4 {
  const double *nx, *ny, *nz, *nw;
  const uint8_t *mark;
  const float4 *shadow;
  const float *spp;
  const unsigned long long *absmax;
  const int *rows, *n_rows;
  int nq, k;
  double ox, oy, oz, ow;
  SelfWrap wr;                   // thr_gt = +Inf: no copy is skipped, and the rows' first tau
  int32_t *idx, *count;
  double *key;
};

__global__ __launch_bounds__(kSelfThreads) void closest_rows4_kernel(const ClosestRows4 a) {
  __shared__ float4 tile[2][kSelfTile];
  __shared__ float tilep[2][kSelfTile];
  __shared__ double4 rowg[kSelfWaves][kSelfSlots];        // the copies of the wave's row sample
  __shared__ QRecF4 rowf[kSelfWaves][kSelfSlots];         // ... and their screen records for the row's tau
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nr = min(max(*a.n_rows, 0), a.nq);
  const int G = (nr + kClosestGroup - 1) / kClosestGroup;
  if ((int)blockIdx.x >= G) return;                         // (workgroup-uniform)
  const int g = G - 1 - (int)blockIdx.x;                    // heaviest group first
  const double C = __longlong_as_double((long long)*a.absmax);
  const unsigned long long kmask = lanes_below(a.k);        // (k <= 32)
  // the wave's row: sample, copies, the pairs held (pair l in lane l), tau and the tau the screen records were made for
  const int c = g * kClosestGroup + wave;
  int j = c < nr ? a.rows[c] : -1;
  if ((unsigned)j >= (unsigned)a.nq) j = -1;
  j = __builtin_amdgcn_readfirstlane(j);
  const int ns = j >= 0 ? 1 << min(max(a.wr.n_wraps, 0), 3) : 0;      // a wave without a row screens and tests nothing
  int cnt = 0, bi = -1;
  // tau starts at +Inf, taken from the launch's thr_gt: a kernel argument, not a literal.  (As a literal the compiler keeps
  // it in a scalar pair set by one s_mov_b64 with a 64-bit immediate, which gfx950 cannot encode -- the assembler refuses
  // that line of the compiler's own listing -- and the kernel then ran with tau = 0: every row came back empty.)
  double bs = __builtin_inf(), tau = a.wr.thr_gt, tauf = tau;
  if (lane < ns) {
    const double p[4] = {a.nx[j], a.ny[j], a.nz[j], a.nw[j]};
    double gc[4];
    (void)self_copy(a.wr, p, lane, gc);
    QRec4 q4;
    q4.x = gc[0]; q4.y = gc[1]; q4.z = gc[2]; q4.w = gc[3]; q4.thr = tau; q4.pad0 = 0.0; q4.pad1 = 0.0; q4.pad2 = 0.0;
    rowg[wave][lane] = make_double4(gc[0], gc[1], gc[2], gc[3]);
    rowf[wave][lane] = make_qrecf<4>(q4, C, a.ox, a.oy, a.oz, a.ow);
  }
  // (the block is the wave's own: the first barrier of the tile loop comes before its first read)
  // the workgroup's last row is the last of its group (the list is ascending): columns 0 .. ncols - 1
  int ncols = a.rows[min(nr, (g + 1) * kClosestGroup) - 1];
  ncols = min(max(ncols, 0), a.nq - 1);
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
    if (tb >= j) continue;                 // (wave-uniform; the barrier above is passed by every wave all the same)
    float x[kScanFU], y[kScanFU], z[kScanFU], w[kScanFU], pp[kScanFU];
#pragma unroll
    for (int u = 0; u < kScanFU; ++u) {
      const float4 cf = tile[buf][u * 64 + lane];
      x[u] = cf.x; y[u] = cf.y; z[u] = cf.z; w[u] = cf.w; pp[u] = tilep[buf][u * 64 + lane];
    }
    // bit u: the lane's column u survived the screen of some copy.  "t > thr'" proves s_slot >= tau (thr' = +Inf while
    // the row is not full, and with a non-finite or huge C: nothing is dropped then); a column is dropped only when
    // every copy proves it, and then min over the slots >= tau
    unsigned sm = 0u;
    for (int sl = 0; sl < ns; ++sl) {
      const QRecF4 rf = rowf[wave][sl];
      float tv[kScanFU];
      screen8<4>(rf, x, y, z, w, pp, tv);
#pragma unroll
      for (int u = 0; u < kScanFU; ++u) sm |= !(tv[u] > rf.thr) ? (1u << u) : 0u;
    }
    if (__ballot(sm != 0u) == 0ull) continue;
#pragma unroll
    for (int u = 0; u < kScanFU; ++u) {
      const bool surv = ((sm >> u) & 1u) != 0u;
      if (__ballot(surv) == 0ull) continue;
      const int i = tb + u * 64 + lane;
      double s = __builtin_inf();
      bool hit = false;
      if (surv && i < j && a.mark[i] == 0) {               // i < j <= nq - 1: inside the table
        const double cx = a.nx[i], cy = a.ny[i], cz = a.nz[i], cw = a.nw[i];
        for (int sl = 0; sl < ns; ++sl) {
          const double4 gc = rowg[wave][sl];
          const double ss = sq4(gc.x, gc.y, gc.z, gc.w, cx, cy, cz, cw);
          s = ss < s ? ss : s;
        }
        hit = s < tau;                                     // (a non-finite s is in no row)
      }
      // the lanes' pairs go in one at a time, ascending in i; each insertion may lower tau and drop the rest
      unsigned long long b = __ballot(hit);
      while (b != 0ull) {
        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)b) - 1);
        const double nsq = wave_read(s, l);
        const int ni = tb + u * 64 + l;
        // the pairs held have lower indices, so the new one goes behind every pair with the same s (lanes k and up
        // hold what fell off the row: not counted, never read)
        const int pos = __popcll(__ballot(bs <= nsq) & kmask);
        const double us = wave_shift_up(bs);
        const int ui = wave_shift_up(bi);
        if (lane > pos) { bs = us; bi = ui; }
        else if (lane == pos) { bs = nsq; bi = ni; }
        cnt = min(cnt + 1, a.k);
        if (cnt == a.k) tau = wave_read(bs, a.k - 1);
        hit = hit && lane != l && s < tau;
        b = __ballot(hit);
      }
    }
    // the screen records follow tau once a tile: a stale (higher) tau only lets more pairs through to the exact test.
    // (The wave's own block, and its next read lies behind the next tile's barrier.)
    if (tau != tauf) {
      tauf = tau;
      if (lane < ns) {
        const double4 gc = rowg[wave][lane];
        QRec4 q4;
        q4.x = gc.x; q4.y = gc.y; q4.z = gc.z; q4.w = gc.w; q4.thr = tau; q4.pad0 = 0.0; q4.pad1 = 0.0; q4.pad2 = 0.0;
        rowf[wave][lane] = make_qrecf<4>(q4, C, a.ox, a.oy, a.oz, a.ow);
      }
    }
  }
  if (j < 0) return;
  if (lane < cnt) {
    a.idx[(size_t)j * a.k + lane] = bi;
    a.key[(size_t)j * a.k + lane] = sqrt_rn(bs);
  }
  if (lane == 0) a.count[j] = cnt;
}

}  // namespace

int launch_closest_self(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, int k, double robot_radius,
                        const uint8_t *skip_dev, const uint8_t *want_dev, int32_t *count_dev, const TreeColumn &tree) {
  if (nq <= 0) return RRTX_OK;
  const ClosestSelfBlock B{(size_t)nq, (size_t)k, false};   // ws_self (block_layout.hpp); L.owner holds B.owner_bytes
  const size_t n = B.n, cap = B.slots;
  RRTX_HIP(ctx, ctx->ws_self.ensure(B.bytes));
  void *ws = ctx->ws_self.p;
  double4 *tab = B.tab.in_as<double4>(ws);
  float4 *shadow = B.shadow.in_as<float4>(ws);
  int64_t *slots_off = B.slots_off.in(ws), *rows_off = B.rows_off.in(ws);
  unsigned long long *absmax = B.absmax.in(ws);
  int32_t *row_owner = B.row_owner.in(ws), *tree_near = tree.tree_idx ? B.tree_near.in(ws) : nullptr;
  RRTX_HIP(ctx, hipMemsetAsync(absmax, 0, sizeof(unsigned long long), ctx->stream));
  ClosestPlan p;
  p.tab = tab; p.want = want_dev; p.tree_idx = tree.tree_idx; p.nq = nq; p.k = k;
  p.rows = B.rows.in(ws); p.n_rows = B.n_rows.in(ws); p.tree_near = tree_near;
  p.slots_end = slots_off + n; p.rows_end = rows_off + n;
  ClosestRows a;
  a.tab = tab; a.shadow = shadow; a.absmax = absmax; a.rows = p.rows; a.n_rows = p.n_rows; a.nq = nq; a.k = k;
  a.ox = ctx->origin[0]; a.oy = ctx->origin[1]; a.oz = ctx->origin[2];
  a.idx = L.idx; a.count = count_dev; a.cost = L.key;
  span_begin(ctx, KF_NN_SCAN);
  hipLaunchKernelGGL(self_table_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, q_dev, nq, skip_dev,
                     a.ox, a.oy, a.oz, tab, shadow, absmax);
  hipLaunchKernelGGL(closest_fill_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, ctx->stream, nq, k, L.idx,
                     L.key, L.e.hit_out, L.e.hit_in, count_dev, L.owner, row_owner, tree.e.hit_out, tree.e.hit_in);
  hipLaunchKernelGGL(closest_plan_kernel, dim3(1), dim3(kPlanThreads), 0, ctx->stream, p);
  hipLaunchKernelGGL(closest_rows_kernel, dim3((unsigned)((nq + kClosestGroup - 1) / kClosestGroup)), dim3(kSelfThreads), 0,
                     ctx->stream, a);
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  // both directed edges of every slot against the WHOLE obstacle list (r < 0), by the kernels of rrtx_extend_candidates:
  // slot e = (row e / k, sample idx[e]); an empty slot (idx -1) and everything past the last filled row is left alone
  Lists slots = L;
  slots.offsets = slots_off; slots.cap = (int64_t)cap;
  int rc = launch_list_edges(ctx, slots, q_dev, nq, robot_radius, 0.0, -1.0, NearTable{B.tab.in(ws), nq});
  if (rc || !tree.tree_idx) return rc;
  // the tree column: one entry a row, (row j, node tree_idx[j]); an index outside the tree is left alone by the kernels
  if (ctx->n_nodes <= 0 || !ctx->nodes_aos) return RRTX_OK;
  return launch_list_edges(ctx, Lists{rows_off, nullptr, tree_near, row_owner, nullptr, tree.e, nq}, q_dev, nq, robot_radius, 0.0,
                           -1.0);
}

int launch_closest_self_dubins(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, int k, double robot_radius,
                               double r_min, const uint8_t *skip_dev, const uint8_t *want_dev, int32_t *count_dev,
                               const TreeColumn &tree) {
  if (nq <= 0) return RRTX_OK;
  const ClosestSelfBlock B{(size_t)nq, (size_t)k, true};   // ws_self (block_layout.hpp); L.owner holds B.owner_bytes
  const size_t n = B.n, cap = B.slots;
  RRTX_HIP(ctx, ctx->ws_self.ensure(B.bytes));
  void *ws = ctx->ws_self.p;
  double *col = B.tab.in(ws);
  float4 *shadow = B.shadow.in_as<float4>(ws);
  float *spp = B.spp.in(ws);
  uint8_t *mark = B.mark.in(ws);
  int64_t *slots_off = B.slots_off.in(ws), *rows_off = B.rows_off.in(ws);
  unsigned long long *absmax = B.absmax.in(ws);
  int32_t *row_owner = B.row_owner.in(ws), *tree_near = tree.tree_idx ? B.tree_near.in(ws) : nullptr;
  RRTX_HIP(ctx, hipMemsetAsync(absmax, 0, sizeof(unsigned long long), ctx->stream));
  ClosestPlan4 p;
  p.mark = mark; p.want = want_dev; p.tree_idx = tree.tree_idx; p.nq = nq; p.k = k;
  p.rows = B.rows.in(ws); p.n_rows = B.n_rows.in(ws); p.tree_near = tree_near;
  p.slots_end = slots_off + n; p.rows_end = rows_off + n;
  ClosestRows4 a;
  a.nx = col; a.ny = col + n; a.nz = col + 2 * n; a.nw = col + 3 * n;
  a.mark = mark; a.shadow = shadow; a.spp = spp; a.absmax = absmax; a.rows = p.rows; a.n_rows = p.n_rows;
  a.nq = nq; a.k = k;
  a.ox = ctx->origin[0]; a.oy = ctx->origin[1]; a.oz = ctx->origin[2]; a.ow = ctx->origin[3];
  a.wr.n_wraps = ctx->n_wraps;
  for (int w = 0; w < 3; ++w) { a.wr.wd[w] = ctx->wrap_dim[w]; a.wr.wp[w] = ctx->wrap_period[w]; }
  a.wr.thr_gt = __builtin_inf();             // no copy is skipped, so C covers every copy of every live sample; the first tau
  a.idx = L.idx; a.count = count_dev; a.key = L.key;
  span_begin(ctx, KF_NN_SCAN);
  hipLaunchKernelGGL(self_table4_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, q_dev, nq, skip_dev,
                     a.wr, a.ox, a.oy, a.oz, a.ow, col, col + n, col + 2 * n, col + 3 * n, mark, shadow, spp, absmax);
  hipLaunchKernelGGL(closest_fill4_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, ctx->stream, nq, k, L.idx,
                     L.key, L.e.cost_out, L.e.cost_in, L.e.word_out, L.e.word_in, L.e.hit_out, L.e.hit_in, count_dev,
                     L.owner, row_owner, tree.e.cost_out, tree.e.cost_in, tree.e.word_out, tree.e.word_in, tree.e.hit_out,
                     tree.e.hit_in);
  hipLaunchKernelGGL(closest_plan4_kernel, dim3(1), dim3(kPlanThreads), 0, ctx->stream, p);
  hipLaunchKernelGGL(closest_rows4_kernel, dim3((unsigned)((nq + kClosestGroup - 1) / kClosestGroup)), dim3(kSelfThreads), 0,
                     ctx->stream, a);
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  // both directed Dubins edges of every slot, by the kernels of rrtx_extend_candidates_dubins: slot e = (row e / k, sample
  // idx[e]) with the sample columns as the near table; an empty slot (idx -1) and everything past the last filled row is
  // left alone
  Lists slots = L;
  slots.offsets = slots_off; slots.cap = (int64_t)cap;
  int rc = launch_candidate_dubins(ctx, slots, q_dev, nq, r_min, robot_radius, NearTable{col, nq});
  if (rc || !tree.tree_idx) return rc;
  // the tree column: one entry a row, (row j, node tree_idx[j]); an index outside the tree is left alone by the kernels
  if (ctx->n_nodes <= 0 || !ctx->nodes[0]) return RRTX_OK;
  return launch_candidate_dubins(ctx, Lists{rows_off, nullptr, tree_near, row_owner, nullptr, tree.e, nq}, q_dev, nq, r_min,
                                 robot_radius);
}

int launch_self_join(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, double r, const uint8_t *skip_dev,
                     NearTable *table_out) {
  if (nq <= 0) return RRTX_OK;
  const SelfJoinBlock B{(size_t)nq, false};   // ws_self (block_layout.hpp)
  RRTX_HIP(ctx, ctx->ws_self.ensure(B.bytes));
  void *ws = ctx->ws_self.p;
  double4 *tab = B.tab.in_as<double4>(ws);
  float4 *shadow = B.shadow.in_as<float4>(ws);
  int *count = B.count.in(ws);
  unsigned long long *absmax = B.absmax.in(ws);
  RRTX_HIP(ctx, hipMemsetAsync(absmax, 0, sizeof(unsigned long long), ctx->stream));
  SelfJoin a;
  a.tab = tab; a.shadow = shadow; a.absmax = absmax; a.nq = nq;
  a.thr = thr_first_ge(r);
  a.ox = ctx->origin[0]; a.oy = ctx->origin[1]; a.oz = ctx->origin[2];
  a.count = count; a.offsets = L.offsets; a.cap = (long long)L.cap;
  a.idx = L.idx; a.owner = L.owner; a.cost = L.key;
  const int G = (nq + kSelfGroup - 1) / kSelfGroup;
  const dim3 grid((unsigned)((G + 1) / 2));
  span_begin(ctx, KF_NN_SCAN);
  hipLaunchKernelGGL(self_table_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, q_dev, nq, skip_dev,
                     a.ox, a.oy, a.oz, tab, shadow, absmax);
  hipLaunchKernelGGL(self_join_kernel<false>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  launch_excl_scan<int64_t>(ctx->stream, count, L.offsets, nq, L.count);
  if (L.cap > 0) hipLaunchKernelGGL(self_join_kernel<true>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  if (table_out) *table_out = NearTable{B.tab.in(ws), nq};
  return RRTX_OK;
}

int launch_self_join_dubins(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, double r, const uint8_t *skip_dev,
                            NearTable *table_out) {
  if (nq <= 0) return RRTX_OK;
  const SelfJoinBlock B{(size_t)nq, true};   // ws_self (block_layout.hpp)
  const size_t n = B.n;
  RRTX_HIP(ctx, ctx->ws_self.ensure(B.bytes));
  void *ws = ctx->ws_self.p;
  double *col = B.tab.in(ws);
  unsigned long long *absmax = B.absmax.in(ws);
  RRTX_HIP(ctx, hipMemsetAsync(absmax, 0, sizeof(unsigned long long), ctx->stream));
  SelfJoin4 a;
  a.nx = col; a.ny = col + n; a.nz = col + 2 * n; a.nw = col + 3 * n;
  a.mark = B.mark.in(ws); a.shadow = B.shadow.in_as<float4>(ws); a.spp = B.spp.in(ws);
  a.absmax = absmax; a.nq = nq;
  a.thr = thr_first_ge(r);
  a.ox = ctx->origin[0]; a.oy = ctx->origin[1]; a.oz = ctx->origin[2]; a.ow = ctx->origin[3];
  a.wr.n_wraps = ctx->n_wraps;
  for (int w = 0; w < 3; ++w) { a.wr.wd[w] = ctx->wrap_dim[w]; a.wr.wp[w] = ctx->wrap_period[w]; }
  a.wr.thr_gt = thr_first_gt(r);
  a.count = B.count.in(ws); a.offsets = L.offsets; a.cap = (long long)L.cap;
  a.idx = L.idx; a.owner = L.owner; a.key = L.key;
  const int G = (nq + kSelfGroup - 1) / kSelfGroup;
  const dim3 grid((unsigned)((G + 1) / 2));
  span_begin(ctx, KF_NN_SCAN);
  hipLaunchKernelGGL(self_table4_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, ctx->stream, q_dev, nq, skip_dev,
                     a.wr, a.ox, a.oy, a.oz, a.ow, col, col + n, col + 2 * n, col + 3 * n,
                     B.mark.in(ws), B.shadow.in_as<float4>(ws), B.spp.in(ws), absmax);
  hipLaunchKernelGGL(self_join4_kernel<false>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  launch_excl_scan<int64_t>(ctx->stream, a.count, L.offsets, nq, L.count);
  if (L.cap > 0) hipLaunchKernelGGL(self_join4_kernel<true>, grid, dim3(kSelfThreads), 0, ctx->stream, a);
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  if (table_out) *table_out = NearTable{col, nq};
  return RRTX_OK;
}

}  // namespace rrtx
