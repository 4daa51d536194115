// kernels_link.hip -- the neighbour lists of an extend batch become edges of the mirror, on the device
// (rrtx_graph_edges_append_lists*, rrtx_graph_edges_append_selected), and the read-back of mirror edges
// (rrtx_graph_edges_get).
//
// Semantics (include/rrtx.h): for j = 0 .. nq-1 with v = node_of[j] >= 0, in that order, and for every surviving entry e
// of row j in list order (u = idx[e], or node_of[idx[e]] for lists among the batch; an entry whose mapped value is
// negative does not survive): the out-edge v -> u, always (dist0 = cost_out[e], dist = cost_out[e] or +Inf when
// hit_out[e] != 0), then the in-edge u -> v when hit_in[e] == 0 (dist = dist0 = cost_in[e]).  Edge ids are consecutive
// from the mirror's count, in exactly that order.
//
// Layout, as in kernels_select.hip: the rows are dealt to sub-wave groups sized from the mean row length (list_walk.hpp).
//   link_count_kernel   per row the edges it yields (wave_sum over the group); every index is checked here and the
//                       verdict ORed into one word, the surviving entries summed into another.
//   excl_scan_kernel    (wave_device.hpp) one workgroup: row_first[nq + 1] and the total.
//   (the host reads entries, edges and the verdict -- 24 bytes -- refuses or grows the mirror)
//   link_fill_kernel    the same walk; two ballots over the group's lanes give every surviving entry its slot: entries
//                       below it plus in-edges below it.  Plain vector stores, no atomic on the placement: an id never
//                       depends on the order in which waves run.  No write lands at or beyond `limit`.
// Inside the entry loops only ballots are used, which count active lanes only.
#include "list_walk.hpp"

namespace rrtx {
namespace {

struct LinkArgs {
  int nq;
  const int64_t *offsets;
  const int32_t *idx;
  const double *cost_out, *cost_in;
  const uint8_t *hit_out, *hit_in;
  const int64_t *n_valid;      // entries the extend call produced (null: not checked)
  long long cap;               // entries the list arrays hold
  const int32_t *node_of;      // nq: node index of sample j, negative: not inserted
  int idx_is_batch;
  long long n_nodes;
  int *row_cnt;                // workspace, nq: edges of every row
  int64_t *row_first;          // nq + 1: exclusive scan of row_cnt
  int64_t *res;                // [0] surviving entries, [1] edges (the scan's total), [2] verdict (kLink* bits)
  // the fill: the mirror's arrays, the id of the batch's first edge, one past its last
  int32_t *ge_start, *ge_end;
  double *ge_dist, *ge_dist0;
  uint8_t *ge_dirty;
  long long first, limit;
};

// the near node of entry value i: -1 dropped (self lists), -2 out of range
__device__ __forceinline__ int link_near(const LinkArgs &a, int i, unsigned &bad) {
  if (a.idx_is_batch) {
    if ((unsigned)i >= (unsigned)a.nq) { bad |= kLinkBadIndex; return -2; }
    const int u = a.node_of[i];
    if (u < 0) return -1;
    if (u >= a.n_nodes) { bad |= kLinkBadNode; return -2; }
    return u;
  }
  if ((unsigned long long)(long long)i >= (unsigned long long)a.n_nodes) { bad |= kLinkBadIndex; return -2; }
  return i;
}

// row s as the two kernels walk it: its node (negative: the row yields nothing) and its entries
__device__ __forceinline__ int link_row(const LinkArgs &a, long long s, long long &beg, long long &end, unsigned &bad) {
  beg = 0; end = 0;
  if (s >= a.nq) return -1;
  const long long b = a.offsets[s], e = a.offsets[s + 1];
  if (b < 0 || b > e || e > a.cap) { bad |= kLinkBadOffsets; return -1; }
  const int v = a.node_of[s];
  if (v < 0) return -1;
  if (v >= a.n_nodes) { bad |= kLinkBadNode; return -1; }
  beg = b; end = e;
  return v;
}

__global__ __launch_bounds__(kWalkBlock) void link_count_kernel(LinkArgs a) {
  if (a.n_valid && *a.n_valid > a.cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr((unsigned long long *)(a.res + 2), (unsigned long long)kLinkOverflow);
    for (long long s = (long long)blockIdx.x * kWalkBlock + threadIdx.x; s < a.nq; s += (long long)gridDim.x * kWalkBlock)
      a.row_cnt[s] = 0;
    return;
  }
  const WalkLanes w = walk_lanes(walk_group(a.offsets, a.nq));
  unsigned bad = 0;
  long long entries = 0;
  for (long long s0 = w.first; s0 < a.nq; s0 += w.stride) {
    const long long s = s0 + w.lane / w.g;
    long long beg, end;
    link_row(a, s, beg, end, bad);
    long long cnt = 0, ent = 0;
    for (long long e = beg + w.sub; e < end; e += w.g) {
      if (link_near(a, a.idx[e], bad) < 0) continue;
      ++ent;
      cnt += a.hit_in[e] == 0 ? 2 : 1;
    }
    cnt = wave_sum(cnt, w.g);
    entries += ent;
    if (cnt > 0x7fffffffll) { bad |= kLinkTooMany; cnt = 0; }
    if (s < a.nq && w.sub == 0) a.row_cnt[s] = (int)cnt;
  }
  entries = wave_sum(entries);
  if (w.lane == 0 && entries) atomicAdd((unsigned long long *)a.res, (unsigned long long)entries);
  if (bad) atomicOr((unsigned long long *)(a.res + 2), (unsigned long long)bad);   // (a refusal: rare, any order)
}

__global__ __launch_bounds__(kWalkBlock) void link_fill_kernel(LinkArgs a) {
  const WalkLanes w = walk_lanes(walk_group(a.offsets, a.nq));
  const unsigned long long group_mask = lane_group_mask(w.lane, w.g);
  const unsigned long long below = group_mask & lanes_below(w.lane);
  for (long long s0 = w.first; s0 < a.nq; s0 += w.stride) {
    const long long s = s0 + w.lane / w.g;
    long long beg, end;
    unsigned bad = 0;
    const int v = link_row(a, s, beg, end, bad);
    if (v < 0) continue;
    long long at = a.first + a.row_first[s];
    for (long long e0 = beg; e0 < end; e0 += w.g) {
      const long long e = e0 + w.sub;
      int u = -1;
      bool both = false;
      if (e < end) {
        u = link_near(a, a.idx[e], bad);
        both = u >= 0 && a.hit_in[e] == 0;
      }
      const bool take = u >= 0;
      const unsigned long long votes = __ballot(take) & group_mask;
      const unsigned long long pairs = __ballot(both) & group_mask;
      if (take) {
        const long long o = at + __popcll(votes & below) + __popcll(pairs & below);
        if (o >= a.first && o + (both ? 1 : 0) < a.limit) {
          const double co = a.cost_out[e];
          a.ge_start[o] = v; a.ge_end[o] = u;
          a.ge_dist0[o] = co;
          a.ge_dist[o] = a.hit_out[e] == 0 ? co : __builtin_huge_val();
          a.ge_dirty[o] = 0;
          if (both) {
            const double ci = a.cost_in[e];
            a.ge_start[o + 1] = u; a.ge_end[o + 1] = v;
            a.ge_dist0[o + 1] = ci;
            a.ge_dist[o + 1] = ci;
            a.ge_dirty[o + 1] = 0;
          }
        }
      }
      at += __popcll(votes) + __popcll(pairs);
    }
  }
}

// mirror edges ids[i] (validated by the caller; an id outside [0, ne) is skipped all the same): any output may be null
__global__ void link_gather_kernel(const int32_t *__restrict__ ids, long long n, long long ne, const int32_t *__restrict__ es,
                                   const int32_t *__restrict__ ee, const double *__restrict__ dist,
                                   const double *__restrict__ dist0, int32_t *__restrict__ o_start, int32_t *__restrict__ o_end,
                                   double *__restrict__ o_dist, double *__restrict__ o_dist0) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long e = ids[i];
  if (e < 0 || e >= ne) return;
  if (o_start) o_start[i] = es[e];
  if (o_end) o_end[i] = ee[e];
  if (o_dist) o_dist[i] = dist[e];
  if (o_dist0) o_dist0[i] = dist0[e];
}

LinkArgs link_args(rrtx_ctx *ctx, const LinkLists &L) {
  LinkArgs a;
  a.nq = L.nq;
  const ListsRO &V = L.lists;
  a.offsets = V.offsets; a.idx = V.idx; a.cost_out = V.e.cost_out; a.cost_in = V.e.cost_in;
  a.hit_out = V.e.hit_out; a.hit_in = V.e.hit_in;
  a.n_valid = V.count; a.cap = (long long)V.cap;
  a.node_of = L.node_of; a.idx_is_batch = L.idx_is_batch ? 1 : 0;
  a.n_nodes = (long long)ctx->n_nodes;
  a.row_cnt = ctx->ws_link_cnt.as<int>();
  a.row_first = L.row_first;
  a.res = ctx->ws_link_res.as<int64_t>();
  a.ge_start = nullptr; a.ge_end = nullptr; a.ge_dist = nullptr; a.ge_dist0 = nullptr; a.ge_dirty = nullptr;
  a.first = 0; a.limit = 0;
  return a;
}

}  // namespace

// the counting pass and the scan; ctx->ws_link_res then holds {surviving entries, edges, verdict}
int launch_link_count(rrtx_ctx *ctx, const LinkLists &L) {
  if (L.nq <= 0) return RRTX_OK;
  RRTX_HIP(ctx, ctx->ws_link_cnt.ensure(sizeof(int) * (size_t)L.nq));
  RRTX_HIP(ctx, ctx->ws_link_res.ensure(sizeof(int64_t) * 3));
  RRTX_HIP(ctx, hipMemsetAsync(ctx->ws_link_res.p, 0, sizeof(int64_t) * 3, ctx->stream));
  const LinkArgs a = link_args(ctx, L);
  hipLaunchKernelGGL(link_count_kernel, dim3(walk_blocks(L.nq)), dim3(kWalkBlock), 0, ctx->stream, a);
  launch_excl_scan(ctx->stream, a.row_cnt, a.row_first, a.nq, a.res + 1);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

// the fill: `total` edges from id `first` on; the mirror's arrays hold at least first + total edges
int launch_link_fill(rrtx_ctx *ctx, const LinkLists &L, long long first, long long total) {
  if (L.nq <= 0 || total <= 0) return RRTX_OK;
  if (first < 0 || first + total > ctx->ge_cap) return fail(ctx, RRTX_E_STATE, "link_fill: edges beyond the mirror's capacity");
  LinkArgs a = link_args(ctx, L);
  a.ge_start = ctx->ge_start; a.ge_end = ctx->ge_end; a.ge_dist = ctx->ge_dist; a.ge_dist0 = ctx->ge_dist0;
  a.ge_dirty = ctx->ge_dirty;
  a.first = first; a.limit = first + total;
  hipLaunchKernelGGL(link_fill_kernel, dim3(walk_blocks(L.nq)), dim3(kWalkBlock), 0, ctx->stream, a);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

int launch_link_gather(rrtx_ctx *ctx, const int32_t *ids_dev, long long n, int32_t *start_dev, int32_t *end_dev,
                       double *dist_dev, double *dist0_dev) {
  if (n <= 0) return RRTX_OK;
  hipLaunchKernelGGL(link_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ids_dev, n,
                     (long long)ctx->ge_n, ctx->ge_start, ctx->ge_end, ctx->ge_dist, ctx->ge_dist0, start_dev, end_dev, dist_dev,
                     dist0_dev);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

}  // namespace rrtx
