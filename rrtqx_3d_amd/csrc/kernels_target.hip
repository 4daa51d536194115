// kernels_target.hip -- findNewTarget (R/DRRT_Q.jl:2901-2994) for a batch of robot poses: the neighbour with the lowest
// rrtLMC + edge.dist among the safe edges pose -> neighbour, the search ball doubling until one exists or the ball
// exceeds the world.  One ROUND = one range search + candidate-edge pass over the poses still searching (the existing
// launchers, per-pose thresholds) followed by the two kernels here; the lists never leave the device.
//
// Semantics (exact: every output is an input value, an index, ONE rounded fp64 addition or r0 * 2^j):
//   select   best = +Inf; for every entry e of the pose in list order with hit_out[e] == 0:
//            cand = lmc[idx[e]] + cost[e]; adopt when best > cand.  A NaN or +Inf candidate is never adopted, and of
//            exactly equal candidates the lowest list position (= lowest node index) wins.
//   advance  a pose without a target doubles its radius; beyond r_max it leaves as RRTX_TGT_NOT_FOUND with the last
//            radius searched, otherwise it moves, in order, into the next round's query block.
//
// Layout.  target_select_kernel deals the poses to sub-wave groups of 8, 16, 32 or 64 lanes sized from the mean list
// length (as select_parent_kernel does); a lane keeps the first minimum of its own entries, the group reduces
// (value, position) lexicographically by butterfly exchange: no atomics.  target_advance_kernel is ONE workgroup: it
// counts the poses that go on, compacts them in order (ballot + wave sums) and forms their thresholds
// min{s : sqrt(s) >= 2r} / > 2r with the stepping of the host's thr_first_ge (fp64 sqrt is correctly rounded on
// gfx950, tests/test_gpu_parity.py::test_device_sqrt_div), so the host reads back three words per round.
// Every index is checked before it is used: list positions against cap, node indices against the length of lmc,
// pose slots against nq.
#include "exact_math.hpp"
#include "rrtx_internal.hpp"

namespace rrtx {
namespace {

constexpr int kTgtBlock = 256;
constexpr int kTgtWave = 64;
constexpr int kAdvBlock = 1024;

__device__ __forceinline__ bool tgt_overflow(const TargetRound &a) { return *a.n_valid > a.cap || *a.n_valid < 0; }

// lanes per pose: the smallest of 8, 16, 32, 64 that covers the mean list length
__device__ __forceinline__ int tgt_group(const TargetRound &a) {
  long long total = a.offsets[a.n_act];
  if (total < 0) total = 0;
  const long long mean = total / (a.n_act > 0 ? a.n_act : 1);
  int g = 8;
  while (g < kTgtWave && g < mean) g <<= 1;
  return g;
}

__device__ __forceinline__ double tgt_lmc(const TargetRound &a, int j) {
  return ((unsigned long long)(long long)j < (unsigned long long)a.n_lmc) ? a.lmc[j] : __builtin_huge_val();
}

__global__ __launch_bounds__(kTgtBlock) void target_select_kernel(TargetRound a) {
  if (tgt_overflow(a)) return;
  const int g = tgt_group(a);
  const int lane = threadIdx.x & (kTgtWave - 1);
  const int sub = lane & (g - 1);
  const long long stride = (long long)gridDim.x * kTgtBlock / g;
  for (long long s0 = ((long long)blockIdx.x * kTgtBlock + (threadIdx.x - lane)) / g; s0 < a.n_act; s0 += stride) {
    const long long s = s0 + lane / g;
    const bool live = s < a.n_act;
    long long beg = 0, end = 0;
    if (live) {
      long long b = a.offsets[s], e = a.offsets[s + 1];
      if (e > a.cap) e = a.cap;
      if (b >= 0 && b <= e) { beg = b; end = e; }
    }
    double best = __builtin_huge_val();
    int pos = 0x7fffffff;
    for (long long e = beg + sub; e < end; e += g) {
      if (a.hit_out[e] != 0) continue;
      const double cand = tgt_lmc(a, a.idx[e]) + a.cost[e];
      if (best > cand) { best = cand; pos = (int)(e - beg); }
    }
    for (int off = g >> 1; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off);
      const int op = __shfl_xor(pos, off);
      if (ov < best || (ov == best && op < pos)) { best = ov; pos = op; }
    }
    if (live && sub == 0) {
      const int o = a.slot[s];
      const bool ok = pos != 0x7fffffff;
      int pend = -1;                                  // (a slot outside the call is dropped)
      if ((unsigned)o < (unsigned)a.nq) {
        if (ok) {
          a.target_idx[o] = a.idx[beg + pos];
          a.edge_dist[o] = a.cost[beg + pos];
          a.cost_to_goal[o] = best;
          a.radius_used[o] = a.rad[s];
          a.rounds[o] = a.round;
          a.status[o] = RRTX_TGT_OK;
        } else {
          const long long len = end - beg;
          pend = len > 0x7fffffffll ? 0x7fffffff : (int)len;
        }
      }
      a.pending[s] = pend;
    }
  }
}

// first s >= 0 for which pred holds, pred monotone over the non-negative doubles: thr_first_ge / thr_first_gt of
// rrtx_capi.hip, step for step (r finite and positive here)
template <bool GT>
__device__ __forceinline__ bool tgt_pred(double s, double r) { return GT ? sqrt_rn(s) > r : sqrt_rn(s) >= r; }

template <bool GT>
__device__ double tgt_first_true(double r) {
  double s = r * r;
  for (int it = 0; it < 16; ++it) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(s);
    if (tgt_pred<GT>(s, r)) {
      if (s == 0.0) return 0.0;
      const double p = __longlong_as_double((long long)(b - 1ull));
      if (!tgt_pred<GT>(p, r)) return s;
      s = p;
    } else {
      if (b == 0x7ff0000000000000ull) return __builtin_nan("");
      const double n = __longlong_as_double((long long)(b + 1ull));
      if (tgt_pred<GT>(n, r)) return n;
      s = n;
    }
  }
  unsigned long long lo = 0ull, hi = 0x7ff0000000000000ull;
  if (tgt_pred<GT>(0.0, r)) return 0.0;
  if (!tgt_pred<GT>(__longlong_as_double((long long)hi), r)) return __builtin_nan("");
  while (hi - lo > 1ull) {
    const unsigned long long mid = lo + (hi - lo) / 2ull;
    if (tgt_pred<GT>(__longlong_as_double((long long)mid), r)) hi = mid; else lo = mid;
  }
  return __longlong_as_double((long long)hi);
}

// a pose that found no target goes on when twice its radius is still within r_max
__device__ __forceinline__ bool tgt_goes_on(const TargetRound &a, int s) {
  return a.pending[s] >= 0 && !(a.rad[s] * 2.0 > a.r_max);
}

__global__ __launch_bounds__(kAdvBlock) void target_advance_kernel(TargetRound a) {
  const int t = threadIdx.x, lane = t & (kTgtWave - 1), w = t / kTgtWave;
  if (tgt_overflow(a)) {                              // the host grows the lists and runs the round again
    if (t == 0) { a.hdr[1] = -1; a.hdr[2] = 0; }
    return;
  }
  __shared__ int wave_cnt[kAdvBlock / kTgtWave];
  __shared__ long long wave_ent[kAdvBlock / kTgtWave];
  int c = 0;
  for (int s = t; s < a.n_act; s += kAdvBlock) c += tgt_goes_on(a, s) ? 1 : 0;
  for (int off = kTgtWave >> 1; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (lane == 0) wave_cnt[w] = c;
  __syncthreads();
  int n_next = 0;
  for (int k = 0; k < kAdvBlock / kTgtWave; ++k) n_next += wave_cnt[k];
  __syncthreads();

  int carry = 0;
  long long ent = 0;
  for (int base = 0; base < a.n_act; base += kAdvBlock) {
    const int s = base + t;
    const bool pend = s < a.n_act && a.pending[s] >= 0;
    const bool on = pend && tgt_goes_on(a, s);
    if (pend && !on) {
      const int o = a.slot[s];
      if ((unsigned)o < (unsigned)a.nq) {
        a.target_idx[o] = -1;
        a.edge_dist[o] = __builtin_huge_val();
        a.cost_to_goal[o] = __builtin_huge_val();
        a.radius_used[o] = a.rad[s];
        a.rounds[o] = a.round;
        a.status[o] = RRTX_TGT_NOT_FOUND;
      }
    }
    const unsigned long long votes = __ballot(on);
    if (lane == 0) wave_cnt[w] = __popcll(votes);
    __syncthreads();
    int before = carry, chunk = 0;
    for (int k = 0; k < kAdvBlock / kTgtWave; ++k) {
      if (k < w) before += wave_cnt[k];
      chunk += wave_cnt[k];
    }
    if (on) {
      const int p = before + __popcll(votes & ((1ull << lane) - 1ull));
      if (p < n_next) {
        const double r2 = a.rad[s] * 2.0;
        for (int k = 0; k < a.dim; ++k) a.q_next[(long long)p * a.dim + k] = a.q[(long long)s * a.dim + k];
        a.slot_next[p] = a.slot[s];
        a.rad_next[p] = r2;
        a.thr_next[p] = tgt_first_true<false>(r2);
        a.thr_next[n_next + p] = tgt_first_true<true>(r2);
        ent += a.pending[s];
      }
    }
    carry += chunk;
    __syncthreads();
  }
  for (int off = kTgtWave >> 1; off > 0; off >>= 1) ent += __shfl_xor(ent, off);
  if (lane == 0) wave_ent[w] = ent;
  __syncthreads();
  if (t == 0) {
    long long tot = 0;
    for (int k = 0; k < kAdvBlock / kTgtWave; ++k) tot += wave_ent[k];
    a.hdr[1] = n_next;
    a.hdr[2] = tot;
  }
}

}  // namespace

int launch_target_round(rrtx_ctx *ctx, const TargetRound &T) {
  if (T.n_act <= 0) return RRTX_OK;
  // a group of 32 lanes per pose fills the device once; beyond that the groups stride
  long long blocks = ((long long)T.n_act * 32 + kTgtBlock - 1) / kTgtBlock;
  blocks = std::max(1ll, std::min(blocks, 2048ll));
  hipLaunchKernelGGL(target_select_kernel, dim3((unsigned)blocks), dim3(kTgtBlock), 0, ctx->stream, T);
  hipLaunchKernelGGL(target_advance_kernel, dim3(1), dim3(kAdvBlock), 0, ctx->stream, T);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

}  // namespace rrtx
