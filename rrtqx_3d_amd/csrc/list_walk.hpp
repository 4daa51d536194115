// list_walk.hpp -- the walk over per-item neighbour lists (CSR) that findBestParent (kernels_select.hip) and
// findNewTarget (kernels_target.hip) share: items are dealt to sub-wave GROUPS of 8, 16, 32 or 64 lanes -- the smallest
// power of two that covers the mean list length, which every wave reads off offsets[n] -- and a group strides over its
// list, so the reads of one group are contiguous.
//
// The rule both entry points promise (walk_first_min): best = +Inf; for every entry e of the list in order with
// hit[e] == 0: cand = lmc[idx[e]] + cost[e]; adopt when best > cand.  A NaN or +Inf candidate is therefore never
// adopted, and of exactly equal candidates the lowest list position wins.  Every lane keeps the (value, position) of
// the first minimum among its own entries (ascending positions, strict >), the group reduces the pairs
// lexicographically by butterfly exchange: the winner is the lowest position by construction, no atomics.
//
// The item loop is wave-uniform (groups past the last item walk an empty list), so the exchanges run with every lane
// active.  Every index is checked before it is used: list positions against cap, node indices against the length of
// lmc.  Everything here has internal linkage.
#pragma once
#include "rrtx_internal.hpp"
#include "wave_device.hpp"

namespace rrtx {
namespace {

constexpr int kWalkBlock = 256;      // threads per workgroup of a walking kernel
constexpr int kNoPos = 0x7fffffff;   // WalkMin::pos of a list without a finite candidate

// lanes per item: the smallest of 8, 16, 32, 64 that covers the mean list length
__device__ __forceinline__ int walk_group(const int64_t *offsets, int n) {
  long long total = offsets[n];
  if (total < 0) total = 0;
  const long long mean = total / (n > 0 ? n : 1);
  int g = 8;
  while (g < 64 && g < mean) g <<= 1;
  return g;
}

// how a thread takes part: for (s0 = first; s0 < n; s0 += stride) its item is s0 + lane / g, its entries are
// beg + sub, beg + sub + g, ...
struct WalkLanes { int g, lane, sub; long long first, stride; };
__device__ __forceinline__ WalkLanes walk_lanes(int g) {
  WalkLanes w;
  w.g = g;
  w.lane = threadIdx.x & 63;
  w.sub = w.lane & (g - 1);
  w.first = ((long long)blockIdx.x * kWalkBlock + (threadIdx.x - w.lane)) / g;
  w.stride = (long long)gridDim.x * kWalkBlock / g;
  return w;
}

// the list of item s, clipped to what the arrays hold (empty for s >= n and for offsets out of order)
__device__ __forceinline__ void walk_segment(const int64_t *offsets, int n, long long cap, long long s, long long &beg,
                                             long long &end) {
  beg = 0; end = 0;
  if (s >= n) return;
  long long b = offsets[s], e = offsets[s + 1];
  if (e > cap) e = cap;
  if (b < 0 || b > e) return;
  beg = b; end = e;
}

// rrtLMC of node j; +Inf for an index outside the array
__device__ __forceinline__ double walk_lmc(const double *lmc, long long n_lmc, int j) {
  return ((unsigned long long)(long long)j < (unsigned long long)n_lmc) ? lmc[j] : __builtin_huge_val();
}

// the first minimum of lmc[idx[e]] + cost[e] over the unblocked entries of [beg, end), in every lane of the group;
// pos is relative to beg, kNoPos when nothing was adopted
struct WalkMin { double best; int pos; };
__device__ __forceinline__ WalkMin walk_first_min(const WalkLanes &w, long long beg, long long end, const uint8_t *hit,
                                                  const int32_t *idx, const double *cost, const double *lmc,
                                                  long long n_lmc) {
  double best = __builtin_huge_val();
  int pos = kNoPos;
  for (long long e = beg + w.sub; e < end; e += w.g) {
    if (hit[e] != 0) continue;
    const double cand = walk_lmc(lmc, n_lmc, idx[e]) + cost[e];
    if (best > cand) { best = cand; pos = (int)(e - beg); }
  }
  for (int off = w.g >> 1; off > 0; off >>= 1) {
    const double ov = __shfl_xor(best, off);
    const int op = __shfl_xor(pos, off);
    if (ov < best || (ov == best && op < pos)) { best = ov; pos = op; }
  }
  return WalkMin{best, pos};
}

// a group of 32 lanes per item fills the device once (8 waves on each of 1024 SIMDs); beyond that the groups stride
inline unsigned walk_blocks(long long n) {
  const long long blocks = (n * 32 + kWalkBlock - 1) / kWalkBlock;
  return (unsigned)std::max(1ll, std::min(blocks, 2048ll));
}

}  // namespace
}  // namespace rrtx
