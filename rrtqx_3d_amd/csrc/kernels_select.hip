// kernels_select.hip -- findBestParent and the rewire test of extend() over the lists of the fused extend
// preamble (R/DRRT_Q.jl:1927-1979, 2619-2634): per sample the parent that minimises rrtLMC(neighbour) + cost,
// the sample's own rrtLMC, and the neighbours whose rrtLMC the new node would lower.
//
// Semantics (exact: every output is an input value, an index or ONE rounded fp64 addition):
//   parent   best = +Inf; for every entry e of the sample in list order with hit_out[e] == 0:
//            cand = lmc[idx[e]] + cost_out[e]; adopt when best > cand.  A NaN or +Inf candidate is therefore never
//            adopted, and of exactly equal candidates the lowest list position wins.
//   rewire   (only with a parent) every entry with hit_in[e] == 0, idx[e] != parent and
//            lmc[idx[e]] > best + cost_in[e], reported in list order as (idx[e], best + cost_in[e]).
// The lists are against the tree as it stood, exactly as in rrtx_extend_candidates (the samples' lists among
// themselves come from rrtx_extend_candidates_self, kernels_self.hip) -- so a node may appear in the rewire lists of
// several samples; settling that is the caller's bookkeeping.
//
// Layout.  Segments average ~25 entries at C4 size and range from 0 to a few hundred: a wave per sample would idle
// most lanes, a lane per sample would serialise the long lists, so the samples are dealt to sub-wave groups sized from
// the mean segment length (list_walk.hpp, which also holds the parent rule's first-minimum walk).
//   select_parent_kernel  the walk, then a second pass over the segment that counts the sample's rewire entries.
//   excl_scan_kernel      (wave_device.hpp) one workgroup: exclusive scan of the per-sample counts -> rw_offsets,
//                         rw_needed; skipped when the lists overflowed.
//   select_rewire_kernel  the second pass again; a ballot over the group's lanes gives every reported entry its place
//                         behind rw_offsets[s], in list order.  Entries at or beyond rw_cap are not written.
// Inside the entry loops only ballots are used, which count active lanes only.
#include "list_walk.hpp"

namespace rrtx {
namespace {

struct SelArgs {
  int nq;
  const int64_t *offsets;
  const int32_t *idx;
  const double *cost_out, *cost_in;
  const uint8_t *hit_out, *hit_in;
  const int64_t *n_valid;      // entries the extend call produced (null: not checked)
  long long cap;               // entries the list arrays hold
  const uint8_t *unsafe;       // may be null
  const double *lmc;
  long long n_lmc;
  int32_t *parent_idx;
  int64_t *parent_entry;
  double *lmc_new;
  uint8_t *status;
  int *rw_count;               // workspace, nq
  int64_t *rw_offsets;
  int32_t *rw_node;
  double *rw_value;
  long long rw_cap;
  int64_t *rw_needed;
};

__device__ __forceinline__ bool sel_overflow(const SelArgs &a) { return a.n_valid && *a.n_valid > a.cap; }

__device__ __forceinline__ WalkLanes sel_lanes(const SelArgs &a) { return walk_lanes(walk_group(a.offsets, a.nq)); }

__global__ __launch_bounds__(kWalkBlock) void select_parent_kernel(SelArgs a) {
  if (sel_overflow(a)) {
    for (long long s = (long long)blockIdx.x * kWalkBlock + threadIdx.x; s < a.nq; s += (long long)gridDim.x * kWalkBlock)
      a.status[s] = RRTX_SEL_OVERFLOW;
    return;
  }
  const WalkLanes w = sel_lanes(a);
  for (long long s0 = w.first; s0 < a.nq; s0 += w.stride) {
    const long long s = s0 + w.lane / w.g;
    long long beg, end;
    walk_segment(a.offsets, a.nq, a.cap, s, beg, end);
    const bool live = s < a.nq;
    const bool unsafe = live && a.unsafe && a.unsafe[s] != 0;
    if (unsafe) end = beg;
    const WalkMin m = walk_first_min(w, beg, end, a.hit_out, a.idx, a.cost_out, a.lmc, a.n_lmc);
    const bool ok = m.pos != kNoPos;
    const int parent = ok ? a.idx[beg + m.pos] : -1;
    int cnt = 0;
    if (ok)
      for (long long e = beg + w.sub; e < end; e += w.g) {
        if (a.hit_in[e] != 0) continue;
        const int j = a.idx[e];
        if (j == parent) continue;
        if (walk_lmc(a.lmc, a.n_lmc, j) > m.best + a.cost_in[e]) ++cnt;
      }
    cnt = wave_sum(cnt, w.g);
    if (live && w.sub == 0) {
      a.status[s] = unsafe ? RRTX_SEL_UNSAFE : (beg == end ? RRTX_SEL_EMPTY : (ok ? RRTX_SEL_OK : RRTX_SEL_NO_PARENT));
      a.parent_idx[s] = parent;
      a.parent_entry[s] = ok ? beg + m.pos : -1;
      a.lmc_new[s] = m.best;
      a.rw_count[s] = cnt;
    }
  }
}

__global__ __launch_bounds__(kWalkBlock) void select_rewire_kernel(SelArgs a) {
  if (sel_overflow(a)) return;
  const WalkLanes w = sel_lanes(a);
  const unsigned long long group_mask = lane_group_mask(w.lane, w.g);
  const unsigned long long below = group_mask & lanes_below(w.lane);
  for (long long s0 = w.first; s0 < a.nq; s0 += w.stride) {
    const long long s = s0 + w.lane / w.g;
    if (s >= a.nq || a.status[s] != RRTX_SEL_OK) continue;
    long long beg, end;
    walk_segment(a.offsets, a.nq, a.cap, s, beg, end);
    const double best = a.lmc_new[s];
    const int parent = a.parent_idx[s];
    long long at = a.rw_offsets[s];
    for (long long e0 = beg; e0 < end; e0 += w.g) {
      const long long e = e0 + w.sub;
      bool take = false;
      int j = -1;
      double v = 0.0;
      if (e < end && a.hit_in[e] == 0) {
        j = a.idx[e];
        v = best + a.cost_in[e];
        take = j != parent && walk_lmc(a.lmc, a.n_lmc, j) > v;
      }
      const unsigned long long votes = __ballot(take) & group_mask;
      if (take) {
        const long long o = at + __popcll(votes & below);
        if (o >= 0 && o < a.rw_cap) { a.rw_node[o] = j; a.rw_value[o] = v; }
      }
      at += __popcll(votes);
    }
  }
}

__global__ void select_fill_inf_kernel(double *__restrict__ p, long long first, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[first + i] = __builtin_huge_val();
}

}  // namespace

int launch_select(rrtx_ctx *ctx, const SelectLaunch &L) {
  RRTX_HIP(ctx, ctx->ws_sel_cnt.ensure(sizeof(int) * (size_t)(L.nq > 0 ? L.nq : 1)));
  SelArgs a;
  a.nq = L.nq;
  const ListsRO &V = L.lists;
  a.offsets = V.offsets; a.idx = V.idx; a.cost_out = V.e.cost_out; a.cost_in = V.e.cost_in;
  a.hit_out = V.e.hit_out; a.hit_in = V.e.hit_in;
  a.n_valid = V.count; a.cap = (long long)V.cap;
  a.unsafe = L.sample_unsafe; a.lmc = L.lmc; a.n_lmc = (long long)L.n_lmc;
  a.parent_idx = L.parent_idx; a.parent_entry = L.parent_entry; a.lmc_new = L.lmc_new; a.status = L.status;
  a.rw_count = ctx->ws_sel_cnt.as<int>();
  a.rw_offsets = L.rw_offsets; a.rw_node = L.rw_node; a.rw_value = L.rw_value; a.rw_cap = (long long)L.rw_cap;
  a.rw_needed = L.rw_needed_dev;
  const dim3 grid(walk_blocks(L.nq)), block(kWalkBlock);
  if (L.nq > 0) hipLaunchKernelGGL(select_parent_kernel, grid, block, 0, ctx->stream, a);
  launch_excl_scan(ctx->stream, a.rw_count, a.rw_offsets, a.nq, a.rw_needed, a.n_valid, a.cap);
  if (L.nq > 0) hipLaunchKernelGGL(select_rewire_kernel, grid, block, 0, ctx->stream, a);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

// the context's own rrtLMC array: one fp64 per node, +Inf until set
int node_cost_ensure(rrtx_ctx *ctx) {
  const int64_t n = ctx->n_nodes;
  if (n > ctx->node_lmc_cap || !ctx->node_lmc) {
    const int64_t nc = std::max<int64_t>(std::max<int64_t>(ctx->cap_nodes, n), 1024);
    if (int rc = regrow(ctx, ctx->node_lmc, nc, ctx->node_lmc_n)) return rc;
    ctx->node_lmc_cap = nc;
  }
  if (n > ctx->node_lmc_n) {
    const long long m = (long long)(n - ctx->node_lmc_n);
    hipLaunchKernelGGL(select_fill_inf_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, ctx->node_lmc.get(),
                       (long long)ctx->node_lmc_n, m);
    RRTX_HIP(ctx, hipGetLastError());
    ctx->node_lmc_n = n;
  }
  return RRTX_OK;
}

}  // namespace rrtx
