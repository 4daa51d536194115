// wave_device.hpp -- the wave64 and workgroup idioms the small kernels share: the inclusive scan and the sum over a
// wave, the count / rank of a flag over a workgroup, and the exclusive scan of a counter array by one workgroup.
// Every function is called by all lanes of the wave (the workgroup ones by all threads of the workgroup) together.
// Everything here has internal linkage.  gfx950 only (wave64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace rrtx {
namespace {

// inclusive prefix sum over the 64 lanes of a wave (lane = threadIdx.x & 63)
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T o = __shfl_up(v, off);
    if (lane >= off) v += o;
  }
  return v;
}

// sum over aligned groups of `width` lanes (a power of two) by xor butterfly: every lane ends with its group's sum
template <class T>
__device__ __forceinline__ T wave_sum(T v, int width = 64) {
  for (int off = width >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// ---- half waves (32 lanes = two DPP rows of 16) and waves without the LDS crossbar's address arithmetic ----
// All lanes of the wave active.  A DPP move with bound_ctrl and full masks folds into the 32-bit VOP2 instruction that
// uses it (v_sub_u32_dpp, v_min_i32_dpp), so such a step is one instruction where a __shfl step is a clamped lane
// address, a ds_bpermute and a wait; a 64-bit step is two moves and the operation.
template <int CTRL>
__device__ __forceinline__ int dpp_move(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
constexpr int kDppRowShr = 0x110, kDppRowRor = 0x120, kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143;
// the value of lane ^ 16: the other row of the half wave (ds_swizzle, bit mode: and 0x1f, or 0, xor 0x10)
__device__ __forceinline__ int other_row(int v) { return __builtin_amdgcn_ds_swizzle(v, 0x401f); }

// How many of the 32 keys `src` of the half wave are smaller than `mine`, for keys in [0, INT_MAX]: there
// src - mine cannot overflow and its sign bit is the comparison, so a key costs a subtraction that reads its DPP row
// rotation and a funnel shift that collects the sign.  SELF = false leaves the lane's own src out (src == mine).
template <bool SELF>
__device__ __forceinline__ int half_rank_below(int src, int mine) {
  const int oth = other_row(src);
  unsigned ba = 0u, bb = 0u;               // two collectors, taking turns: neither waits for its own last result
#define RRTX_RANK_KEY(bits, o) bits = __builtin_amdgcn_alignbit(bits, (unsigned)((o) - mine), 31u);
#define RRTX_RANK_ROT(bits, v, n) RRTX_RANK_KEY(bits, dpp_move<kDppRowRor + n>(v))
#define RRTX_RANK_ROW(v)                                                                                              \
  RRTX_RANK_ROT(ba, v, 1) RRTX_RANK_ROT(bb, v, 2) RRTX_RANK_ROT(ba, v, 3) RRTX_RANK_ROT(bb, v, 4)                     \
  RRTX_RANK_ROT(ba, v, 5) RRTX_RANK_ROT(bb, v, 6) RRTX_RANK_ROT(ba, v, 7) RRTX_RANK_ROT(bb, v, 8)                     \
  RRTX_RANK_ROT(ba, v, 9) RRTX_RANK_ROT(bb, v, 10) RRTX_RANK_ROT(ba, v, 11) RRTX_RANK_ROT(bb, v, 12)                  \
  RRTX_RANK_ROT(ba, v, 13) RRTX_RANK_ROT(bb, v, 14) RRTX_RANK_ROT(ba, v, 15)
  if (SELF) RRTX_RANK_KEY(bb, src)
  RRTX_RANK_ROW(src)
  RRTX_RANK_KEY(bb, oth)
  RRTX_RANK_ROW(oth)
#undef RRTX_RANK_ROW
#undef RRTX_RANK_ROT
#undef RRTX_RANK_KEY
  return __popc(ba) + __popc(bb);          // 16 bits in ba, 15 or 16 in bb
}

// minimum over the half wave, in every lane of it
__device__ __forceinline__ int half_min(int v) {
  v = min(v, dpp_move<kDppRowRor + 1>(v));
  v = min(v, dpp_move<kDppRowRor + 2>(v));
  v = min(v, dpp_move<kDppRowRor + 4>(v));
  v = min(v, dpp_move<kDppRowRor + 8>(v));
  return min(v, other_row(v));
}
// ... of doubles that are never NaN (a compare and a select: fmin would canonicalise its operands first)
template <int CTRL>
__device__ __forceinline__ double dpp_move_d(double v) {
  const long long b = __double_as_longlong(v);
  const int lo = dpp_move<CTRL>((int)(b & 0xffffffffll)), hi = dpp_move<CTRL>((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo);
}
__device__ __forceinline__ double min_no_nan(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double half_min_no_nan(double v) {
  v = min_no_nan(v, dpp_move_d<kDppRowRor + 1>(v));
  v = min_no_nan(v, dpp_move_d<kDppRowRor + 2>(v));
  v = min_no_nan(v, dpp_move_d<kDppRowRor + 4>(v));
  v = min_no_nan(v, dpp_move_d<kDppRowRor + 8>(v));
  const long long b = __double_as_longlong(v);
  const int lo = other_row((int)(b & 0xffffffffll)), hi = other_row((int)(b >> 32));
  return min_no_nan(v, __longlong_as_double(((long long)hi << 32) | (long long)(unsigned)lo));
}

// 64-bit sums by row shifts and row broadcasts (a lane without a source adds zero):
// the inclusive scan over each row of 16 lanes, and from it the sum over the wave, valid in lane 63 only
#define RRTX_SUM_STEP(ctrl)                                                                                           \
  {                                                                                                                   \
    const unsigned lo = (unsigned)dpp_move<ctrl>((int)(unsigned)(v & 0xffffffffull));                                 \
    const unsigned hi = (unsigned)dpp_move<ctrl>((int)(unsigned)(v >> 32));                                           \
    v += ((unsigned long long)hi << 32) | lo;                                                                         \
  }
__device__ __forceinline__ unsigned long long row_incl_scan(unsigned long long v) {
  RRTX_SUM_STEP(kDppRowShr + 1) RRTX_SUM_STEP(kDppRowShr + 2) RRTX_SUM_STEP(kDppRowShr + 4) RRTX_SUM_STEP(kDppRowShr + 8)
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_last(unsigned long long v) {
  v = row_incl_scan(v);
  RRTX_SUM_STEP(kDppRowBcast15) RRTX_SUM_STEP(kDppRowBcast31)
  return v;
}
#undef RRTX_SUM_STEP

// the lanes below `lane`, and the aligned group of g lanes (a power of two) that holds `lane`, as ballot masks
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ unsigned long long lane_group_mask(int lane, int g) {
  return (g == 64 ? ~0ull : ((1ull << g) - 1ull)) << (lane & ~(g - 1));
}

// ---- a flag per thread over a workgroup of NT threads: how many are set, and how many before mine ----
// block_votes ballots the flag, leaves every wave's count in wcnt[NT / 64] (LDS) and returns the wave's ballot; after
// it, block_votes_total is the workgroup's count and block_votes_before the count in the waves before mine (add
// __popcll(votes & lanes_below(lane)) for a thread's rank).  wcnt may be written again after the next barrier.
template <int NT>
__device__ __forceinline__ unsigned long long block_votes(bool flag, int *wcnt) {
  const unsigned long long votes = __ballot(flag);
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = __popcll(votes);
  __syncthreads();
  return votes;
}
template <int NT>
__device__ __forceinline__ int block_votes_total(const int *wcnt) {
  int c = 0;
  for (int w = 0; w < NT / 64; ++w) c += wcnt[w];
  return c;
}
__device__ __forceinline__ int block_votes_before(const int *wcnt, int wave) {
  int c = 0;
  for (int w = 0; w < wave; ++w) c += wcnt[w];
  return c;
}

// ---- exclusive prefix sum of n counters by ONE workgroup; out[n] = total ----
// 4096 counters a round: every thread takes four neighbouring counters (one 16-byte load, the wave reads 1 KB in a
// row), the waves' sums meet in LDS, the running total carries over.  (A contiguous stretch of n / 1024 counters per
// thread is 64 cache lines per load instruction and two dependent loads per counter: 22 us for the 15 000 counters of a
// 500 k-node slab index.)  out may be in (Out = int): a thread reads its four counters before it writes them, and no
// other thread touches them.  Pointers that are not aligned for the vector access, and the last n % 4 counters, go
// one by one.  total_too (may be null) receives the total as well; with guard given, *guard > guard_max writes nothing.
constexpr int kScanBlock = 1024;

template <class Out>
__global__ __launch_bounds__(kScanBlock) void excl_scan_kernel(const int *in, Out *out, int n, Out *total_too,
                                                               const int64_t *guard, long long guard_max) {
  if (guard && *guard > guard_max) return;
  using Out4 = HIP_vector_type<Out, 4>;
  __shared__ Out wsum[2][kScanBlock / 64];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool vec_in = (reinterpret_cast<uintptr_t>(in) & (sizeof(int4) - 1)) == 0;
  const bool vec_out = (reinterpret_cast<uintptr_t>(out) & (sizeof(Out4) - 1)) == 0;
  Out carry = 0;
  int flip = 0;
  for (long long base = 0; base < n; base += 4 * kScanBlock, flip ^= 1) {
    const long long i = base + 4 * t;
    const bool full = i + 3 < n;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    if (full && vec_in) {
      const int4 v4 = *reinterpret_cast<const int4 *>(in + i);
      c0 = v4.x; c1 = v4.y; c2 = v4.z; c3 = v4.w;
    } else {
      if (i < n) c0 = in[i];
      if (i + 1 < n) c1 = in[i + 1];
      if (i + 2 < n) c2 = in[i + 2];
      if (full) c3 = in[i + 3];
    }
    const Out local = (Out)c0 + c1 + c2 + c3;
    const Out incl = wave_incl_scan(local, lane);
    if (lane == 63) wsum[flip][wave] = incl;
    __syncthreads();                      // (two sets of sums: the next round's writes cannot overtake this round's reads)
    Out prefix = carry + incl - local, total = 0;
#pragma unroll
    for (int w = 0; w < kScanBlock / 64; ++w) {
      const Out x = wsum[flip][w];
      if (w < wave) prefix += x;
      total += x;
    }
    const Out p1 = prefix + c0, p2 = p1 + c1, p3 = p2 + c2;
    if (full && vec_out) {
      Out4 o4;
      o4.x = prefix; o4.y = p1; o4.z = p2; o4.w = p3;
      *reinterpret_cast<Out4 *>(out + i) = o4;
    } else {
      if (i < n) out[i] = prefix;
      if (i + 1 < n) out[i + 1] = p1;
      if (i + 2 < n) out[i + 2] = p2;
      if (full) out[i + 3] = p3;
    }
    carry += total;
  }
  if (t == 0) {
    out[n] = carry;
    if (total_too) *total_too = carry;
  }
}

template <class Out>
inline void launch_excl_scan(hipStream_t st, const int *in, Out *out, int n, Out *total_too = nullptr,
                             const int64_t *guard = nullptr, long long guard_max = 0) {
  hipLaunchKernelGGL(excl_scan_kernel<Out>, dim3(1), dim3(kScanBlock), 0, st, in, out, n, total_too, guard, guard_max);
}

}  // namespace
}  // namespace rrtx
