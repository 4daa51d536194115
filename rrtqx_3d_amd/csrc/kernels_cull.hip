// kernels_cull.hip -- cullCurrentNeighbors over the device mirror of the planner's edges, and the compaction that
// removes what it culled (rrtx_graph_edges_cull / rrtx_graph_edges_compact, include/rrtx.h).
//
// RRT^X bounds every node's degree by dropping, whenever a node is rewired or has its rrtLMC recalculated, the node's
// CURRENT out-neighbours whose edge.dist exceeds the shrinking ball; its INITIAL out-neighbours stay
// (R/DRRT_Q.jl:2388-2403).  Node indices are insertion order and extend() is the only place edges are made: the edge
// new -> neighbour is the new node's initial out-neighbour, neighbour -> new the older node's current one.  So a
// mirrored edge is a current out-edge of its start node iff start < end, and the mirror needs no flag for it.
//
//   cull      one lane per edge: not yet culled, start listed (a byte per node, scattered from the caller's list),
//             start < end, dist > ball (IEEE: NaN stays, +Inf goes, dist == ball stays).  A culled edge gets
//             dist = distOriginal = +Inf, the touched mark of graph_block_kernel with its patch of the in-edge CSR's
//             cost copy, and a byte of its own.  Every other kernel sees an edge that is blocked for good.
//   compact   stable stream compaction over tiles of kCullTile edges: survivors per tile, the one-workgroup exclusive
//             scan of wave_device.hpp, then a scatter of the five mirror arrays and of remap[old] = new (-1: removed)
//             into second buffers that replace the first.  The solver's parent edges and the baseline of the delta
//             report are renumbered through remap by a gather per node.
// The marking pass reads start and end of every edge (8 bytes) and, for the edges with start < end, the culled byte and
// dist (9 more; one byte of the node map with a list), and writes 18 bytes a culled edge.  Compaction reads the culled
// byte twice and the 25 bytes of every survivor, and writes those 25 and 4 bytes of remap an edge.  gfx950 only.
#include "rrtx_internal.hpp"
#include "wave_device.hpp"

namespace rrtx {

namespace {

constexpr int kCullBlock = 256;                      // threads per workgroup of every kernel here
constexpr int kCullRounds = 4;                       // edges per thread of the compaction kernels, kCullBlock apart
constexpr int kCullTile = kCullBlock * kCullRounds;  // edges per workgroup of the compaction kernels
constexpr int kCullWaves = kCullBlock / 64;

inline dim3 grid_for(long long n, int block = kCullBlock) { return dim3((unsigned)((n + block - 1) / block)); }

// map[nodes[i]] = 1 (nodes validated by the caller; a node listed twice writes the same byte twice)
__global__ void cull_node_map_kernel(const int32_t *__restrict__ nodes, long long k, uint8_t *__restrict__ map) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < k) map[nodes[i]] = 1;
}

// the marking pass; map null: every node is listed.  cnt[workgroup] = edges it culled.
__global__ __launch_bounds__(kCullBlock) void cull_mark_kernel(const int32_t *__restrict__ es, const int32_t *__restrict__ ee,
                                                               double *__restrict__ dist, double *__restrict__ dist0,
                                                               uint8_t *__restrict__ dirty, uint8_t *__restrict__ culled,
                                                               const uint8_t *__restrict__ map, long long ne, double ball,
                                                               const int32_t *__restrict__ in_pos, long long in_ne,
                                                               double *__restrict__ in_w, int *__restrict__ cnt) {
  __shared__ int wcnt[kCullWaves];
  const long long e = (long long)blockIdx.x * kCullBlock + threadIdx.x;
  bool c = false;
  if (e < ne) {
    const int32_t s = es[e], t = ee[e];
    c = s < t && culled[e] == 0 && (!map || map[s] != 0) && dist[e] > ball;
    if (c) {
      const double inf = __builtin_inf();
      dist[e] = inf;
      dist0[e] = inf;
      dirty[e] = 1;
      culled[e] = 1;
      if (e < in_ne) in_w[in_pos[e]] = inf;
    }
  }
  block_votes<kCullBlock>(c, wcnt);
  if (threadIdx.x == 0) cnt[blockIdx.x] = block_votes_total<kCullBlock>(wcnt);
}

// a kept solve whose parent forest still uses a culled edge: *bad = 1
__global__ void cull_parent_check_kernel(const int32_t *__restrict__ parent, int n, const uint8_t *__restrict__ culled,
                                         long long ne, int64_t *__restrict__ bad) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool b = false;
  if (v < n) {
    const int32_t p = parent[v];
    b = p != kNoParentEdge && p >= 0 && p < ne && culled[p] != 0;
  }
  if (__ballot(b) != 0ull && (threadIdx.x & 63) == 0) *bad = 1;
}

// survivors per tile
__global__ __launch_bounds__(kCullBlock) void compact_count_kernel(const uint8_t *__restrict__ culled, long long ne,
                                                                   int *__restrict__ cnt) {
  __shared__ int wsum[kCullWaves];
  const long long base = (long long)blockIdx.x * kCullTile + threadIdx.x;
  int local = 0;
#pragma unroll
  for (int r = 0; r < kCullRounds; ++r) {
    const long long e = base + (long long)r * kCullBlock;
    local += (e < ne && culled[e] == 0) ? 1 : 0;
  }
  local = wave_sum(local);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0;
    for (int w = 0; w < kCullWaves; ++w) c += wsum[w];
    cnt[blockIdx.x] = c;
  }
}

struct MirrorCols {
  int32_t *start, *end;
  double *dist, *dist0;
  uint8_t *dirty;
};

// survivor e of tile b goes to pos[b] + its rank inside the tile (ranks follow the edge id: the order is kept); the
// culled bytes of the new mirror are cleared by the caller.  mark_at: the edge id whose new position (the survivors
// before it) the caller wants in *mark_pos -- the first edge the kept solve has not seen.
__global__ __launch_bounds__(kCullBlock) void compact_scatter_kernel(MirrorCols from, const uint8_t *__restrict__ culled,
                                                                     long long ne, const int64_t *__restrict__ pos, MirrorCols to,
                                                                     int32_t *__restrict__ remap, long long mark_at,
                                                                     int64_t *__restrict__ mark_pos) {
  __shared__ int wcnt[kCullRounds][kCullWaves];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long base = (long long)blockIdx.x * kCullTile + t;
  bool keep[kCullRounds];
  unsigned long long votes[kCullRounds];
#pragma unroll
  for (int r = 0; r < kCullRounds; ++r) {
    const long long e = base + (long long)r * kCullBlock;
    keep[r] = e < ne && culled[e] == 0;
    votes[r] = __ballot(keep[r]);
    if (lane == 0) wcnt[r][wave] = __popcll(votes[r]);
  }
  __syncthreads();
  long long before = pos[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kCullRounds; ++r) {
    const long long e = base + (long long)r * kCullBlock;
    long long at = before;
    for (int w = 0; w < kCullWaves; ++w) {
      const int c = wcnt[r][w];
      if (w < wave) at += c;
      before += c;
    }
    at += __popcll(votes[r] & lanes_below(lane));
    if (e < ne) {
      if (e == mark_at) *mark_pos = at;
      remap[e] = keep[r] ? (int32_t)at : -1;
      if (keep[r]) {
        to.start[at] = from.start[e];
        to.end[at] = from.end[e];
        to.dist[at] = from.dist[e];
        to.dist0[at] = from.dist0[e];
        to.dirty[at] = from.dirty[e];
      }
    }
  }
}

// the solver's parent edges through remap (none of them removed: the caller has checked)
__global__ void compact_parent_kernel(int32_t *__restrict__ parent, int n, const int32_t *__restrict__ remap, long long ne) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t p = parent[v];
  if (p != kNoParentEdge && p >= 0 && p < ne) parent[v] = remap[p];
}

// the delta baseline's parent edges (-1: none) through remap; an edge that was removed becomes kRemovedEdge, which no
// id the solver reports equals
__global__ void compact_baseline_kernel(int32_t *__restrict__ base_par, long long n, const int32_t *__restrict__ remap,
                                        long long ne) {
  const long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t p = base_par[v];
  if (p < 0) return;
  const int32_t r = p < ne ? remap[p] : -1;
  base_par[v] = r < 0 ? kRemovedEdge : r;
}

}  // namespace

// nodes_host null: every node.  The caller has validated ball, k and the nodes, and the mirror is not empty.
// Synchronises (the count travels back).
int launch_edges_cull(rrtx_ctx *ctx, double ball, const int32_t *nodes_host, long long k, int64_t *n_culled) {
  const long long ne = ctx->ge_n;
  hipStream_t st = ctx->stream;
  const uint8_t *map = nullptr;
  if (nodes_host) {
    RRTX_HIP(ctx, ctx->ws_cull_map.ensure((size_t)ctx->n_nodes));
    RRTX_HIP(ctx, ctx->ws_cull_nodes.ensure(sizeof(int32_t) * (size_t)k));
    RRTX_HIP(ctx, hipMemsetAsync(ctx->ws_cull_map.p, 0, (size_t)ctx->n_nodes, st));
    RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_cull_nodes.p, nodes_host, sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(cull_node_map_kernel, grid_for(k), dim3(kCullBlock), 0, st, ctx->ws_cull_nodes.as<int32_t>(), k,
                       ctx->ws_cull_map.as<uint8_t>());
    map = ctx->ws_cull_map.as<uint8_t>();
  }
  const int nb = (int)((ne + kCullBlock - 1) / kCullBlock);
  RRTX_HIP(ctx, ctx->ws_cull_cnt.ensure(sizeof(int) * (size_t)nb));
  RRTX_HIP(ctx, ctx->ws_cull_pos.ensure(sizeof(int64_t) * ((size_t)nb + 2)));
  int64_t *pos = ctx->ws_cull_pos.as<int64_t>();
  hipLaunchKernelGGL(cull_mark_kernel, dim3(nb), dim3(kCullBlock), 0, st, ctx->ge_start, ctx->ge_end, ctx->ge_dist, ctx->ge_dist0,
                     ctx->ge_dirty, ctx->ge_culled, map, ne, ball, ctx->gc.in_pos.as<int32_t>(), (long long)ctx->gc.in_ne,
                     ctx->gc.in_w.as<double>(), ctx->ws_cull_cnt.as<int>());
  launch_excl_scan(st, ctx->ws_cull_cnt.as<int>(), pos, nb);
  RRTX_HIP(ctx, hipGetLastError());
  int64_t total = 0;
  RRTX_HIP(ctx, hipMemcpyAsync(&total, pos + nb, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  RRTX_HIP(ctx, hipStreamSynchronize(st));      // (nodes_host is the caller's, too)
  if (total > 0) ctx->gc.touched_old = true;
  if (n_culled) *n_culled = total;
  return RRTX_OK;
}

// remap_host: room for ge_n int32, or null.  RRTX_E_STATE, with nothing changed, when a kept solve has a culled parent
// edge.  Synchronises.
int launch_edges_compact(rrtx_ctx *ctx, int32_t *remap_host, int64_t *n_removed) {
  GraphCost &gc = ctx->gc;
  const long long ne = ctx->ge_n;
  hipStream_t st = ctx->stream;
  const bool kept = gc.solved_root >= 0 && gc.solved_nodes > 0;
  const int nt = (int)((ne + kCullTile - 1) / kCullTile);
  RRTX_HIP(ctx, ctx->ws_cull_cnt.ensure(sizeof(int) * (size_t)nt));
  RRTX_HIP(ctx, ctx->ws_cull_pos.ensure(sizeof(int64_t) * ((size_t)nt + 2)));
  RRTX_HIP(ctx, ctx->ws_cull_res.ensure(sizeof(int64_t) * 2));      // [0] a culled parent edge, [1] new solved_edges
  int64_t *pos = ctx->ws_cull_pos.as<int64_t>(), *res = ctx->ws_cull_res.as<int64_t>();
  RRTX_HIP(ctx, hipMemsetAsync(res, 0, sizeof(int64_t) * 2, st));
  if (kept)
    hipLaunchKernelGGL(cull_parent_check_kernel, grid_for(gc.solved_nodes), dim3(kCullBlock), 0, st, gc.parent.as<int32_t>(),
                       (int)gc.solved_nodes, ctx->ge_culled, ne, res);
  hipLaunchKernelGGL(compact_count_kernel, dim3(nt), dim3(kCullBlock), 0, st, ctx->ge_culled, ne, ctx->ws_cull_cnt.as<int>());
  launch_excl_scan(st, ctx->ws_cull_cnt.as<int>(), pos, nt);
  RRTX_HIP(ctx, hipGetLastError());
  int64_t bad = 0, left = 0;
  RRTX_HIP(ctx, hipMemcpyAsync(&bad, res, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  RRTX_HIP(ctx, hipMemcpyAsync(&left, pos + nt, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  RRTX_HIP(ctx, hipStreamSynchronize(st));
  if (bad)
    return fail(ctx, RRTX_E_STATE, "graph_edges_compact: the kept cost solve still has a culled edge as a parent edge "
                                   "(run rrtx_graph_cost_update first)");
  if (left == ne) {                                  // nothing to remove: the identity
    if (remap_host)
      for (long long e = 0; e < ne; ++e) remap_host[e] = (int32_t)e;
    return RRTX_OK;
  }
  // the second buffers, as large as the first; every allocation before the first write
  DevArray<int32_t> start2, end2;
  DevArray<double> dist2, dist02;
  DevArray<uint8_t> dirty2, culled2;
  int rc;
  if ((rc = regrow(ctx, start2, ctx->ge_cap, 0))) return rc;
  if ((rc = regrow(ctx, end2, ctx->ge_cap, 0))) return rc;
  if ((rc = regrow(ctx, dist2, ctx->ge_cap, 0))) return rc;
  if ((rc = regrow(ctx, dist02, ctx->ge_cap, 0))) return rc;
  if ((rc = regrow(ctx, dirty2, ctx->ge_cap, 0))) return rc;
  if ((rc = regrow(ctx, culled2, ctx->ge_cap, 0))) return rc;
  RRTX_HIP(ctx, ctx->ws_cull_remap.ensure(sizeof(int32_t) * (size_t)ne));
  int32_t *remap = ctx->ws_cull_remap.as<int32_t>();
  RRTX_HIP(ctx, hipMemsetAsync(culled2.get(), 0, (size_t)ctx->ge_cap, st));
  const long long mark_at = kept && gc.solved_edges < ne ? (long long)gc.solved_edges : -1;
  hipLaunchKernelGGL(compact_scatter_kernel, dim3(nt), dim3(kCullBlock), 0, st,
                     MirrorCols{ctx->ge_start, ctx->ge_end, ctx->ge_dist, ctx->ge_dist0, ctx->ge_dirty}, ctx->ge_culled, ne, pos,
                     MirrorCols{start2, end2, dist2, dist02, dirty2}, remap, mark_at, res + 1);
  RRTX_HIP(ctx, hipGetLastError());
  int64_t new_solved = 0;
  RRTX_HIP(ctx, hipMemcpyAsync(&new_solved, res + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (remap_host) RRTX_HIP(ctx, hipMemcpyAsync(remap_host, remap, sizeof(int32_t) * (size_t)ne, hipMemcpyDeviceToHost, st));
  RRTX_HIP(ctx, hipStreamSynchronize(st));
  // Up to here nothing the context keeps has changed.  From here on nothing can be refused: the solver state is
  // renumbered in place behind the scatter (stream order), and should a launch fail all the same, the solve and the
  // baseline are forgotten rather than left half renumbered.
  if (kept)
    hipLaunchKernelGGL(compact_parent_kernel, grid_for(gc.solved_nodes), dim3(kCullBlock), 0, st, gc.parent.as<int32_t>(),
                       (int)gc.solved_nodes, remap, ne);
  if (gc.rep_root >= 0 && gc.rep_nodes > 0)
    hipLaunchKernelGGL(compact_baseline_kernel, grid_for(gc.rep_nodes), dim3(kCullBlock), 0, st, gc.rep_parent.as<int32_t>(),
                       (long long)gc.rep_nodes, remap, ne);
  const hipError_t gathered = hipGetLastError();
  // the second buffers become the mirror (the first are released with the locals)
  std::swap(ctx->ge_start, start2);
  std::swap(ctx->ge_end, end2);
  std::swap(ctx->ge_dist, dist2);
  std::swap(ctx->ge_dist0, dist02);
  std::swap(ctx->ge_dirty, dirty2);
  std::swap(ctx->ge_culled, culled2);
  ctx->ge_n = left;
  if (kept) gc.solved_edges = mark_at >= 0 ? new_solved : left;
  gc.in_ne = 0;                                      // the in-edge CSR holds old ids: the next solve builds it again
  gc.in_nn = 0;
  if (n_removed) *n_removed = ne - left;
  if (gathered != hipSuccess) {
    graph_cost_forget(ctx);
    graph_delta_forget(ctx);
    return fail(ctx, RRTX_E_DEVICE, "graph_edges_compact: renumbering the solver state failed (%s); the mirror is compacted, "
                                    "the kept solve and the delta baseline are forgotten", hipGetErrorString(gathered));
  }
  return RRTX_OK;
}

}  // namespace rrtx
