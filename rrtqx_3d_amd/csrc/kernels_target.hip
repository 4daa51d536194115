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
// Layout.  target_select_kernel is the first-minimum walk of list_walk.hpp (the one select_parent_kernel runs) followed
// by the pose's outputs.  target_advance_kernel is ONE workgroup: it counts the poses that go on, compacts them in order
// (block_votes of wave_device.hpp) and forms their thresholds min{s : sqrt(s) >= 2r} / > 2r with the host's own
// sq_first_ge / sq_first_gt (exact_math.hpp; fp64 sqrt is correctly rounded on gfx950,
// tests/test_gpu_parity.py::test_device_sqrt_div), so the host reads back three words per round.
// Every index is checked before it is used: list positions against cap, node indices against the length of lmc,
// pose slots against nq.
#include "exact_math.hpp"
#include "list_walk.hpp"

namespace rrtx {
namespace {

constexpr int kAdvBlock = 1024;

__device__ __forceinline__ bool tgt_overflow(const TargetRound &a) { return *a.n_valid > a.cap || *a.n_valid < 0; }

__global__ __launch_bounds__(kWalkBlock) void target_select_kernel(TargetRound a) {
  if (tgt_overflow(a)) return;
  const WalkLanes w = walk_lanes(walk_group(a.offsets, a.n_act));
  for (long long s0 = w.first; s0 < a.n_act; s0 += w.stride) {
    const long long s = s0 + w.lane / w.g;
    long long beg, end;
    walk_segment(a.offsets, a.n_act, a.cap, s, beg, end);
    const WalkMin m = walk_first_min(w, beg, end, a.hit_out, a.idx, a.cost, a.lmc, a.n_lmc);
    if (s < a.n_act && w.sub == 0) {
      const int o = a.slot[s];
      int pend = -1;                                  // (a slot outside the call is dropped)
      if ((unsigned)o < (unsigned)a.nq) {
        if (m.pos != kNoPos) {
          a.target_idx[o] = a.idx[beg + m.pos];
          a.edge_dist[o] = a.cost[beg + m.pos];
          a.cost_to_goal[o] = m.best;
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

// a pose that found no target goes on when twice its radius is still within r_max
__device__ __forceinline__ bool tgt_goes_on(const TargetRound &a, int s) {
  return a.pending[s] >= 0 && !(a.rad[s] * 2.0 > a.r_max);
}

__global__ __launch_bounds__(kAdvBlock) void target_advance_kernel(TargetRound a) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (tgt_overflow(a)) {                              // the host grows the lists and runs the round again
    if (t == 0) { a.hdr[1] = -1; a.hdr[2] = 0; }
    return;
  }
  __shared__ int wave_cnt[kAdvBlock / 64];
  __shared__ long long wave_ent[kAdvBlock / 64];
  int c = 0;
  for (int s = t; s < a.n_act; s += kAdvBlock) c += tgt_goes_on(a, s) ? 1 : 0;
  c = wave_sum(c);
  if (lane == 0) wave_cnt[w] = c;
  __syncthreads();
  const int n_next = block_votes_total<kAdvBlock>(wave_cnt);
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
    const unsigned long long votes = block_votes<kAdvBlock>(on, wave_cnt);
    if (on) {
      const int p = carry + block_votes_before(wave_cnt, w) + __popcll(votes & lanes_below(lane));
      if (p < n_next) {
        const double r2 = a.rad[s] * 2.0;
        for (int k = 0; k < a.dim; ++k) a.q_next[(long long)p * a.dim + k] = a.q[(long long)s * a.dim + k];
        a.slot_next[p] = a.slot[s];
        a.rad_next[p] = r2;
        a.thr_next[p] = sq_first_ge(r2);
        a.thr_next[n_next + p] = sq_first_gt(r2);
        ent += a.pending[s];
      }
    }
    carry += block_votes_total<kAdvBlock>(wave_cnt);
    __syncthreads();
  }
  ent = wave_sum(ent);
  if (lane == 0) wave_ent[w] = ent;
  __syncthreads();
  if (t == 0) {
    long long tot = 0;
    for (int k = 0; k < kAdvBlock / 64; ++k) tot += wave_ent[k];
    a.hdr[1] = n_next;
    a.hdr[2] = tot;
  }
}

}  // namespace

int launch_target_round(rrtx_ctx *ctx, const TargetRound &T) {
  if (T.n_act <= 0) return RRTX_OK;
  hipLaunchKernelGGL(target_select_kernel, dim3(walk_blocks(T.n_act)), dim3(kWalkBlock), 0, ctx->stream, T);
  hipLaunchKernelGGL(target_advance_kernel, dim3(1), dim3(kAdvBlock), 0, ctx->stream, T);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

}  // namespace rrtx
