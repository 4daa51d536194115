// kernels_sweep.hip -- the edge loop of addNewObstacle (R/DRRT_Q.jl:3195-3290) against a device
// mirror of the planner's directed edges: nodes within the search range of the obstacle centre
// (findPointsInConflictWithObstacle = kdFindWithinRange with the root's <=), every mirrored edge
// that starts at such a node, explicitEdgeCheck(S, edge, ob) against that one obstacle.
// Returns the ids of the colliding edges in ascending order.  gfx950 only.
#include "collide_device.hpp"
#include "wave_device.hpp"

namespace rrtx {

namespace {

// nodes in range of the obstacle centre: dist < range, the root with <= (thresholds on the squared
// distance, see rrtx_sq_thresholds)
__global__ void sweep_mark_kernel(const double *__restrict__ nx, const double *__restrict__ ny,
                                  const double *__restrict__ nz, int n, double cx, double cy, double cz,
                                  double thr_lt, double thr_gt, uint8_t *__restrict__ mark) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double s = sq3(cx, cy, cz, nx[i], ny[i], nz[i]);
  mark[i] = ((s < thr_lt) || (i == 0 && s < thr_gt)) ? 1 : 0;
}

constexpr int kSweepBlock = 1024;

// flag[e] = edge e starts at a marked node and collides with the obstacle; per-block counts
__global__ __launch_bounds__(kSweepBlock) void sweep_edges_kernel(
    const int32_t *__restrict__ e_start, const int32_t *__restrict__ e_end, long long ne, int n_nodes,
    const uint8_t *__restrict__ mark, const double *__restrict__ naos, SphRec ob, int active,
    uint8_t *__restrict__ flag, int *__restrict__ block_count) {
  __shared__ int wcnt[kSweepBlock / 64];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool hit = false;
  if (e < ne) {
    const int a = e_start[e], b = e_end[e];
    if ((unsigned)a < (unsigned)n_nodes && (unsigned)b < (unsigned)n_nodes && mark[a] && active) {
      const double4 p0 = reinterpret_cast<const double4 *>(naos)[a];
      const double4 p1 = reinterpret_cast<const double4 *>(naos)[b];
      const double len = sqrt_rn(sq3(p0.x, p0.y, p0.z, p1.x, p1.y, p1.z));
      hit = edge_hits_sphere(p0.x, p0.y, p0.z, p1.x - p0.x, p1.y - p0.y, p1.z - p0.z, len, ob);
    }
    flag[e] = hit ? 1 : 0;
  }
  block_votes<kSweepBlock>(hit, wcnt);
  if (threadIdx.x == 0) block_count[blockIdx.x] = block_votes_total<kSweepBlock>(wcnt);
}

// ---- polygon / Dubins space (R/DRRT.jl:3048-3290) ----
// findPointsInConflictWithObstacle there is one range query (static obstacle) or one per path segment (kinds 6 / 7,
// accumulated with kdFindMoreWithinRange), each with its ghosts in wrapped dimensions: a node is in the list when
// ANY of them finds it -- dist < range, the root with <= for the un-wrapped query points (kdTree_general.jl:896,
// 934) and < for the ghosts.  thr_root is the root's threshold (= thr_lt where the root gets no <=).
__global__ void sweep_mark_multi_kernel(const double *__restrict__ nx, const double *__restrict__ ny,
                                        const double *__restrict__ nz, const double *__restrict__ nw, int n, int dim,
                                        const SweepQuery *__restrict__ qs, int nqs, uint8_t *__restrict__ mark) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = nx[i], y = ny[i], z = nz[i], w = (dim == 4) ? nw[i] : 0.0;
  bool in = false;
  for (int k = 0; k < nqs; ++k) {
    const SweepQuery q = qs[k];
    const double s = (dim == 4) ? sq4(q.x, q.y, q.z, q.w, x, y, z, w) : sq3(q.x, q.y, q.z, x, y, z);
    in = in || (s < q.thr_lt) || (i == 0 && s < q.thr_root);
  }
  mark[i] = in ? 1 : 0;
}

// flag[e] = edge e of the mirror starts at a marked node (and, blocked_only: edge.dist == Inf); per-block counts
__global__ __launch_bounds__(kSweepBlock) void sweep_select_kernel(const int32_t *__restrict__ e_start, long long ne,
                                                                   int n_nodes, const uint8_t *__restrict__ mark,
                                                                   const double *__restrict__ e_dist, int blocked_only,
                                                                   uint8_t *__restrict__ flag, int *__restrict__ block_count) {
  __shared__ int wcnt[kSweepBlock / 64];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool sel = false;
  if (e < ne) {
    const int a = e_start[e];
    sel = (unsigned)a < (unsigned)n_nodes && mark[a] != 0 && (!blocked_only || e_dist[e] == __builtin_inf());
    flag[e] = sel ? 1 : 0;
  }
  block_votes<kSweepBlock>(sel, wcnt);
  if (threadIdx.x == 0) block_count[blockIdx.x] = block_votes_total<kSweepBlock>(wcnt);
}

// flag[k] = hit[k] and none of the "other obstacle" results (may be null); per-block counts
__global__ __launch_bounds__(kSweepBlock) void sweep_combine_kernel(const uint8_t *__restrict__ hit, const uint8_t *__restrict__ o1,
                                                                    const uint8_t *__restrict__ o2, long long n,
                                                                    uint8_t *__restrict__ flag, int *__restrict__ block_count) {
  __shared__ int wcnt[kSweepBlock / 64];
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool f = false;
  if (k < n) {
    f = hit[k] != 0 && !(o1 && o1[k] != 0) && !(o2 && o2[k] != 0);
    flag[k] = f ? 1 : 0;
  }
  block_votes<kSweepBlock>(f, wcnt);
  if (threadIdx.x == 0) block_count[blockIdx.x] = block_votes_total<kSweepBlock>(wcnt);
}

// start / end rows (dim doubles each) of the mirrored edges ids[k]
__global__ void sweep_gather_kernel(const int32_t *__restrict__ ids, long long n, const int32_t *__restrict__ es,
                                    const int32_t *__restrict__ ee, const double *__restrict__ naos, int dim,
                                    double *__restrict__ p0, double *__restrict__ p1) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int id = ids[k];
  const double4 a = reinterpret_cast<const double4 *>(naos)[es[id]], b = reinterpret_cast<const double4 *>(naos)[ee[id]];
  p0[dim * k] = a.x; p0[dim * k + 1] = a.y; p0[dim * k + 2] = a.z;
  p1[dim * k] = b.x; p1[dim * k + 1] = b.y; p1[dim * k + 2] = b.z;
  if (dim == 4) { p0[dim * k + 3] = a.w; p1[dim * k + 3] = b.w; }
}

// flagged positions, ascending: block offset + rank inside the block; ids (may be null) maps a position to what is written
__global__ __launch_bounds__(kSweepBlock) void sweep_write_kernel(const uint8_t *__restrict__ flag, long long ne,
                                                                  const long long *__restrict__ block_start,
                                                                  int32_t *__restrict__ out, long long cap,
                                                                  const int32_t *__restrict__ ids = nullptr) {
  __shared__ int wcnt[kSweepBlock / 64];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool hit = e < ne && flag[e] != 0;
  const unsigned long long m = block_votes<kSweepBlock>(hit, wcnt);
  if (!hit) return;
  const long long pos = block_start[blockIdx.x] + block_votes_before(wcnt, threadIdx.x >> 6) + __popcll(m & lanes_below(threadIdx.x & 63));
  if (pos < cap) out[pos] = ids ? ids[e] : (int32_t)e;
}

// ---- the batched sweep (rrtx_obstacle_sweep_batch): up to 64 obstacles a pass over the nodes and over the mirror ----
constexpr int kSweepGroup = 64;      // obstacles per pass: one bit each of a 64-bit word

// word[i] bit b = node i is in range of obstacle b of the group and that obstacle is in use (sweep_mark_kernel's test)
__global__ void sweep_mark_words_kernel(const double *__restrict__ nx, const double *__restrict__ ny,
                                        const double *__restrict__ nz, int n, const SweepObs *__restrict__ tab, int kg,
                                        unsigned long long *__restrict__ word) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = nx[i], y = ny[i], z = nz[i];
  unsigned long long w = 0ull;
  for (int b = 0; b < kg; ++b) {
    const SweepObs o = tab[b];                                   // (uniform: scalar loads)
    const double s = sq3(o.ob.cx, o.ob.cy, o.ob.cz, x, y, z);
    if (((s < o.thr_lt) || (i == 0 && s < o.thr_gt)) && o.active) w |= 1ull << b;
  }
  word[i] = w;
}

// The head of the two passes over the mirror: the hit word of edge e (< ne) against the group.  An edge whose start node
// has an empty word is done after that read; any other loads its endpoints, forms its length once and runs
// edge_hits_sphere for every set bit.  seg = the edge as edge_hits_sphere takes it (untouched where no test ran).
struct EdgeSeg { double ax, ay, az, bx, by, bz, len; };

__device__ __forceinline__ unsigned long long edge_hit_word(const int32_t *__restrict__ e_start, const int32_t *__restrict__ e_end,
                                                            long long e, int n_nodes, const unsigned long long *__restrict__ word,
                                                            const double *__restrict__ naos, const SweepObs *__restrict__ tab,
                                                            EdgeSeg &seg) {
  unsigned long long hits = 0ull;
  const int a = e_start[e];
  unsigned long long w = (unsigned)a < (unsigned)n_nodes ? word[a] : 0ull;
  if (w != 0ull) {
    const int b = e_end[e];
    if ((unsigned)b < (unsigned)n_nodes) {
      const double4 p0 = reinterpret_cast<const double4 *>(naos)[a];
      const double4 p1 = reinterpret_cast<const double4 *>(naos)[b];
      seg.len = sqrt_rn(sq3(p0.x, p0.y, p0.z, p1.x, p1.y, p1.z));
      seg.ax = p0.x; seg.ay = p0.y; seg.az = p0.z;
      seg.bx = p1.x - p0.x; seg.by = p1.y - p0.y; seg.bz = p1.z - p0.z;
      while (w != 0ull) {
        const int j = __ffsll((long long)w) - 1;                 // (j < kg: the mark kernel sets no other bit)
        w &= w - 1ull;
        if (edge_hits_sphere(seg.ax, seg.ay, seg.az, seg.bx, seg.by, seg.bz, seg.len, tab[j].ob)) hits |= 1ull << j;
      }
    }
  }
  return hits;
}

// The tail of the two passes: the edges with a hit word leave (id, hit word) in the block's own stretch of seg_id /
// seg_word, ascending (rank of the thread among the block's hits); blk_n[block] = how many, cnt[b * nb + block] = how
// many of them hit obstacle b.  wcnt / lw: the block's LDS (kSweepBlock / 64 ints, kSweepBlock words).
__device__ __forceinline__ void block_list_write(unsigned long long hits, long long e, int kg, int nb, int *wcnt,
                                                 unsigned long long *lw, int32_t *__restrict__ seg_id,
                                                 unsigned long long *__restrict__ seg_word, int *__restrict__ blk_n,
                                                 int *__restrict__ cnt) {
  const int t = threadIdx.x;
  const bool any = hits != 0ull;
  const unsigned long long m = block_votes<kSweepBlock>(any, wcnt);
  const int total = block_votes_total<kSweepBlock>(wcnt);
  if (t == 0) blk_n[blockIdx.x] = total;
  if (total == 0) {                                              // (the whole block takes this branch or none of it)
    if (t < kg) cnt[(size_t)t * nb + blockIdx.x] = 0;
    return;
  }
  if (any) {
    const int r = block_votes_before(wcnt, t >> 6) + __popcll(m & lanes_below(t & 63));
    const size_t at = (size_t)blockIdx.x * kSweepBlock + r;
    seg_id[at] = (int32_t)e;
    seg_word[at] = hits;
    lw[r] = hits;
  }
  __syncthreads();
  if (t < kg) {
    int c = 0;
    for (int r = 0; r < total; ++r) c += (int)((lw[r] >> t) & 1ull);
    cnt[(size_t)t * nb + blockIdx.x] = c;
  }
}

// One block of kSweepBlock mirrored edges against the group: head, then tail.
__global__ __launch_bounds__(kSweepBlock) void sweep_edges_words_kernel(
    const int32_t *__restrict__ e_start, const int32_t *__restrict__ e_end, long long ne, int n_nodes,
    const unsigned long long *__restrict__ word, const double *__restrict__ naos, const SweepObs *__restrict__ tab, int kg,
    int nb, int32_t *__restrict__ seg_id, unsigned long long *__restrict__ seg_word, int *__restrict__ blk_n,
    int *__restrict__ cnt) {
  __shared__ int wcnt[kSweepBlock / 64];
  __shared__ unsigned long long lw[kSweepBlock];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  EdgeSeg seg;
  const unsigned long long hits = e < ne ? edge_hit_word(e_start, e_end, e, n_nodes, word, naos, tab, seg) : 0ull;
  block_list_write(hits, e, kg, nb, wcnt, lw, seg_id, seg_word, blk_n, cnt);
}

// The rows of one group out of the blocks' lists: pos = exclusive scan of cnt (obstacle-major, so pos[b * nb + block] is
// where block's ids of obstacle b start inside the group and pos[b * nb] where row b starts), *base = ids of the groups
// before this one.  One workgroup of 64 per block of edges, thread b walks the block's list for obstacle b: blocks
// ascend with the scan, ids ascend inside a list.  Block 0 also writes the group's offsets and the next group's base.
__global__ __launch_bounds__(kSweepGroup) void sweep_rows_write_kernel(
    const int32_t *__restrict__ seg_id, const unsigned long long *__restrict__ seg_word, const int *__restrict__ blk_n,
    const long long *__restrict__ pos, int nb, int kg, const long long *__restrict__ base, long long *__restrict__ base_next,
    int64_t *__restrict__ offsets, int32_t *__restrict__ out, long long cap) {
  const int t = threadIdx.x;
  const long long b0 = *base;
  if (blockIdx.x == 0) {
    if (t < kg) offsets[t] = b0 + pos[(size_t)t * nb];
    if (t == 0) {
      const long long end = b0 + pos[(size_t)kg * nb];
      offsets[kg] = end;
      *base_next = end;
    }
  }
  const int m = blk_n[blockIdx.x];
  if (m == 0 || t >= kg) return;
  long long p = b0 + pos[(size_t)t * nb + blockIdx.x];
  const size_t at = (size_t)blockIdx.x * kSweepBlock;
  for (int r = 0; r < m; ++r) {
    if ((seg_word[at + r] >> t) & 1ull) {
      if (p < cap) out[p] = seg_id[at + r];
      ++p;
    }
  }
}

// ---- the batched release (rrtx_obstacle_release_batch): the edge loops of a burst of removeObstacle calls ----
// One block of kSweepBlock mirrored edges against a group of leaving obstacles.  An edge that is not blocked
// (dist != Inf: almost every edge) is done after that one coalesced read; a blocked one takes the head to its hit
// word.  Then the test against the spheres that stay (sph / stay / na: the packed in-use records of the edge checks
// and one byte each, 0 = it leaves with this call), dealt across the wave: the lanes with a hit word are taken in
// turn, the edge is broadcast, the 64 lanes hold it against 64 spheres at a time and ballot; an edge some staying
// sphere hits loses its hit word.  Only after that the tail, so sweep_rows_write_kernel finds what the sweep leaves it.
__global__ __launch_bounds__(kSweepBlock) void release_edges_words_kernel(
    const double *__restrict__ e_dist, const int32_t *__restrict__ e_start, const int32_t *__restrict__ e_end, long long ne,
    int n_nodes, const unsigned long long *__restrict__ word, const double *__restrict__ naos,
    const SweepObs *__restrict__ tab, int kg, int nb, const SphRec *__restrict__ sph, const uint8_t *__restrict__ stay, int na,
    int32_t *__restrict__ seg_id, unsigned long long *__restrict__ seg_word, int *__restrict__ blk_n, int *__restrict__ cnt) {
  __shared__ int wcnt[kSweepBlock / 64];
  __shared__ unsigned long long lw[kSweepBlock];
  const int lane = threadIdx.x & 63;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  EdgeSeg seg = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned long long hits = 0ull;
  if (e < ne && e_dist[e] == __builtin_inf()) hits = edge_hit_word(e_start, e_end, e, n_nodes, word, naos, tab, seg);
  unsigned long long todo = __ballot(hits != 0ull);              // (wave-uniform: the loops below do not diverge)
  while (todo != 0ull) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const double sx = __shfl(seg.ax, src), sy = __shfl(seg.ay, src), sz = __shfl(seg.az, src);
    const double tx = __shfl(seg.bx, src), ty = __shfl(seg.by, src), tz = __shfl(seg.bz, src), sl = __shfl(seg.len, src);
    bool kept = false;
    for (int base = 0; base < na && !kept; base += 64) {
      const int j = base + lane;
      const bool h = j < na && stay[j] != 0 && edge_hits_sphere(sx, sy, sz, tx, ty, tz, sl, sph[j]);
      kept = __ballot(h) != 0ull;
    }
    if (kept && lane == src) hits = 0ull;
  }
  block_list_write(hits, e, kg, nb, wcnt, lw, seg_id, seg_word, blk_n, cnt);
}

// ---- the batched polygon sweep (rrtx_obstacle_sweep_polygon_batch): up to 64 list entries a pass, mode 0 ----
// word[i] bit b = some query of entry b of the group finds node i (sweep_mark_multi_kernel's test, query by query; the
// queries of an obstacle that is not in use are not in the table, so its bit is never set)
__global__ void sweep_mark_query_words_kernel(const double *__restrict__ nx, const double *__restrict__ ny,
                                              const double *__restrict__ nz, const double *__restrict__ nw, int n, int dim,
                                              const SweepQueryOwned *__restrict__ qs, int nqs,
                                              unsigned long long *__restrict__ word) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double x = nx[i], y = ny[i], z = nz[i], w = (dim == 4) ? nw[i] : 0.0;
  unsigned long long in = 0ull;
  for (int k = 0; k < nqs; ++k) {
    const SweepQuery q = qs[k].q;                                // (uniform: scalar loads)
    const unsigned long long owner = qs[k].owner;
    const double s = (dim == 4) ? sq4(q.x, q.y, q.z, q.w, x, y, z, w) : sq3(q.x, q.y, q.z, x, y, z);
    if ((s < q.thr_lt) || (i == 0 && s < q.thr_root)) in |= owner;
  }
  word[i] = in;
}

// the word of mirrored edge e's start node (0: past the end of the mirror, or a start index that points nowhere).
// BLOCKED (the release form): and 0 for an edge that is not blocked, e_dist[e] != +Inf -- read first, so almost every
// edge is done after that one coalesced read.
template <bool BLOCKED>
__device__ __forceinline__ unsigned long long edge_start_word(const int32_t *__restrict__ e_start, long long e, long long ne,
                                                              int n_nodes, const unsigned long long *__restrict__ word,
                                                              const double *__restrict__ e_dist) {
  if (e >= ne) return 0ull;
  if constexpr (BLOCKED) {
    if (e_dist[e] != __builtin_inf()) return 0ull;
  }
  const int a = e_start[e];
  return (unsigned)a < (unsigned)n_nodes ? word[a] : 0ull;
}

// The candidates of a group, two launches around the scan of the blocks' counts: an edge whose start node has a word
// (BLOCKED: and that is blocked in the mirror) is a candidate; they leave as (id, word), ascending.  e_dist is read by
// the BLOCKED form only.
template <bool BLOCKED>
__global__ __launch_bounds__(kSweepBlock) void sweep_cand_count_kernel(const int32_t *__restrict__ e_start, long long ne,
                                                                       int n_nodes, const unsigned long long *__restrict__ word,
                                                                       const double *__restrict__ e_dist,
                                                                       int *__restrict__ block_count) {
  __shared__ int wcnt[kSweepBlock / 64];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  block_votes<kSweepBlock>(edge_start_word<BLOCKED>(e_start, e, ne, n_nodes, word, e_dist) != 0ull, wcnt);
  if (threadIdx.x == 0) block_count[blockIdx.x] = block_votes_total<kSweepBlock>(wcnt);
}
template <bool BLOCKED>
__global__ __launch_bounds__(kSweepBlock) void sweep_cand_write_kernel(const int32_t *__restrict__ e_start, long long ne,
                                                                       int n_nodes, const unsigned long long *__restrict__ word,
                                                                       const double *__restrict__ e_dist,
                                                                       const long long *__restrict__ block_start,
                                                                       int32_t *__restrict__ cand_id,
                                                                       unsigned long long *__restrict__ cand_word) {
  __shared__ int wcnt[kSweepBlock / 64];
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long w = edge_start_word<BLOCKED>(e_start, e, ne, n_nodes, word, e_dist);
  const unsigned long long m = block_votes<kSweepBlock>(w != 0ull, wcnt);
  if (w == 0ull) return;
  const long long pos = block_start[blockIdx.x] + block_votes_before(wcnt, threadIdx.x >> 6) + __popcll(m & lanes_below(threadIdx.x & 63));
  cand_id[pos] = (int32_t)e;                                     // (pos < the scan's total <= ne)
  cand_word[pos] = w;
}

// The SimpleEdge check of a group's candidates, one lane per candidate: the edge's two nodes are loaded once ((x, y)
// and, for obstacles that move, the time in z), then the reference's one-obstacle explicitEdgeCheck2D
// (R/DRRT.jl:1523-1653) for every set bit of the candidate's word -- the arithmetic edges_polygons_kernel
// (kernels_collide.hip) runs for one list position: the bounding-circle test, after which a ball (kind 1) is a hit and
// a polygon (kind 3) is one when a side comes within robotRadius; kinds 6 / 7 by edge_hits_moving.  ppos[b] = the packed
// table position of the group's entry b.  The node lists of these sweeps are short, so the lanes stay on their own.
__global__ __launch_bounds__(256) void sweep_polygon_words_kernel(
    const int32_t *__restrict__ cand_id, const unsigned long long *__restrict__ cand_word, long long n_c,
    const int32_t *__restrict__ e_start, const int32_t *__restrict__ e_end, int n_nodes, const double *__restrict__ naos,
    const double *__restrict__ meta, const int32_t *__restrict__ off, const double *__restrict__ vxy,
    const int32_t *__restrict__ path_off, const double *__restrict__ path, const int32_t *__restrict__ ppos,
    double robot_radius, unsigned long long *__restrict__ hit_word) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_c) return;
  const int id = cand_id[c];
  const int a = e_start[id], b = e_end[id];
  unsigned long long hits = 0ull;
  if ((unsigned)a < (unsigned)n_nodes && (unsigned)b < (unsigned)n_nodes) {
    const double4 p0 = reinterpret_cast<const double4 *>(naos)[a];
    const double4 p1 = reinterpret_cast<const double4 *>(naos)[b];
    const double rr2 = robot_radius * robot_radius;
    unsigned long long w = cand_word[c];
    while (w != 0ull) {
      const int bit = __ffsll((long long)w) - 1;
      w &= w - 1ull;
      const int j = ppos[bit];
      const double cx = meta[4 * j + 0], cy = meta[4 * j + 1], rad = meta[4 * j + 2];
      const int kind = (int)meta[4 * j + 3];
      bool h = false;
      if (kind == 6 || kind == 7) {
        h = edge_hits_moving(p0.x, p0.y, p0.z, p1.x, p1.y, p1.z, robot_radius, cx, cy, rad, path + 3 * (size_t)path_off[j],
                             path_off[j + 1] - path_off[j]);
      } else {
        const double dsq = dist_sqrd_point_to_segment(cx, cy, p0.x, p0.y, p1.x, p1.y);
        const double rr = robot_radius + rad;
        if (!(dsq > rr * rr)) {
          if (kind == 1) h = true;
          else if (kind == 3) {
            const int vb = off[j], ve = off[j + 1];
            if (ve - vb >= 2) {                                  // (:1551: fewer than two vertices never collide)
              double Ax = vxy[2 * (ve - 1)], Ay = vxy[2 * (ve - 1) + 1];
              for (int v = vb; v < ve && !h; ++v) {
                const double Bx = vxy[2 * v], By = vxy[2 * v + 1];
                h = segment_dist_sqrd(p0.x, p0.y, p1.x, p1.y, Ax, Ay, Bx, By) < rr2;
                Ax = Bx; Ay = By;
              }
            }
          }
        }
      }
      if (h) hits |= 1ull << bit;
    }
  }
  hit_word[c] = hits;
}

// The one-obstacle test of sweep_polygon_words_kernel's loop body as a function, for the release form below: the
// reference's explicitEdgeCheck2D (R/DRRT.jl:1523-1653) of the edge p0 -> p1 against packed table position j, statement
// for statement what that kernel runs for one set bit.  (sweep_polygon_words_kernel keeps its own copy: calling this
// function from it moved its SGPR count, and mode 0 is to stay the code it was.)
__device__ __forceinline__ bool polygon_hits_edge(const double4 p0, const double4 p1, int j, const double *__restrict__ meta,
                                                  const int32_t *__restrict__ off, const double *__restrict__ vxy,
                                                  const int32_t *__restrict__ path_off, const double *__restrict__ path,
                                                  double robot_radius, double rr2) {
  const double cx = meta[4 * j + 0], cy = meta[4 * j + 1], rad = meta[4 * j + 2];
  const int kind = (int)meta[4 * j + 3];
  bool h = false;
  if (kind == 6 || kind == 7) {
    h = edge_hits_moving(p0.x, p0.y, p0.z, p1.x, p1.y, p1.z, robot_radius, cx, cy, rad, path + 3 * (size_t)path_off[j],
                         path_off[j + 1] - path_off[j]);
  } else {
    const double dsq = dist_sqrd_point_to_segment(cx, cy, p0.x, p0.y, p1.x, p1.y);
    const double rr = robot_radius + rad;
    if (!(dsq > rr * rr)) {
      if (kind == 1) h = true;
      else if (kind == 3) {
        const int vb = off[j], ve = off[j + 1];
        if (ve - vb >= 2) {                                      // (:1551: fewer than two vertices never collide)
          double Ax = vxy[2 * (ve - 1)], Ay = vxy[2 * (ve - 1) + 1];
          for (int v = vb; v < ve && !h; ++v) {
            const double Bx = vxy[2 * v], By = vxy[2 * v + 1];
            h = segment_dist_sqrd(p0.x, p0.y, p1.x, p1.y, Ax, Ay, Bx, By) < rr2;
            Ax = Bx; Ay = By;
          }
        }
      }
    }
  }
  return h;
}

// The same check in the release form (rrtx_obstacle_release_polygon_batch), on polygon_hits_edge: a lane whose hit
// word is not empty then walks the obstacles that stay -- stay[2 r], stay[2 r + 1] = the r-th range [pb, pe) of packed
// positions, n_stay of them, clamped to the na obstacles of the table -- and drops its word at the first one its edge
// collides with: the single mode-1 call's passes over "the packed obstacles before it" and "after it".  A wave without
// a hit skips the walk.
__global__ __launch_bounds__(256) void release_polygon_words_kernel(
    const int32_t *__restrict__ cand_id, const unsigned long long *__restrict__ cand_word, long long n_c,
    const int32_t *__restrict__ e_start, const int32_t *__restrict__ e_end, int n_nodes, const double *__restrict__ naos,
    const double *__restrict__ meta, const int32_t *__restrict__ off, const double *__restrict__ vxy,
    const int32_t *__restrict__ path_off, const double *__restrict__ path, const int32_t *__restrict__ ppos,
    double robot_radius, unsigned long long *__restrict__ hit_word, const int32_t *__restrict__ stay, int n_stay, int na) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_c) return;
  const int id = cand_id[c];
  const int a = e_start[id], b = e_end[id];
  unsigned long long hits = 0ull;
  if ((unsigned)a < (unsigned)n_nodes && (unsigned)b < (unsigned)n_nodes) {
    const double4 p0 = reinterpret_cast<const double4 *>(naos)[a];
    const double4 p1 = reinterpret_cast<const double4 *>(naos)[b];
    const double rr2 = robot_radius * robot_radius;
    unsigned long long w = cand_word[c];
    while (w != 0ull) {
      const int bit = __ffsll((long long)w) - 1;
      w &= w - 1ull;
      if (polygon_hits_edge(p0, p1, ppos[bit], meta, off, vxy, path_off, path, robot_radius, rr2)) hits |= 1ull << bit;
    }
    if (__ballot(hits != 0ull) != 0ull) {
      for (int r = 0; r < n_stay && hits != 0ull; ++r) {
        const int pb = max(stay[2 * r], 0), pe = min(stay[2 * r + 1], na);
        for (int j = pb; j < pe; ++j)
          if (polygon_hits_edge(p0, p1, j, meta, off, vxy, path_off, path, robot_radius, rr2)) { hits = 0ull; break; }
      }
    }
  }
  hit_word[c] = hits;
}

// The tail over a group's candidates: candidate c hands (cand_id[c], its hit word) to block_list_write, which stores
// the id it is given -- here the edge id, not the position.  nb: blocks of this launch.
__global__ __launch_bounds__(kSweepBlock) void sweep_cand_rows_kernel(
    const int32_t *__restrict__ cand_id, const unsigned long long *__restrict__ hit_word, long long n_c, int kg, int nb,
    int32_t *__restrict__ seg_id, unsigned long long *__restrict__ seg_word, int *__restrict__ blk_n, int *__restrict__ cnt) {
  __shared__ int wcnt[kSweepBlock / 64];
  __shared__ unsigned long long lw[kSweepBlock];
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = c < n_c;
  block_list_write(in ? hit_word[c] : 0ull, in ? (long long)cand_id[c] : 0ll, kg, nb, wcnt, lw, seg_id, seg_word, blk_n, cnt);
}

}  // namespace

// device side of rrtx_obstacle_sweep; needed_dev[0] = colliding edges, needed_dev[1] = block count scratch
int launch_obstacle_sweep(rrtx_ctx *ctx, const double centre[3], double thr_lt, double thr_gt, const SphRec &ob,
                          int active, int32_t *out_dev, int64_t cap, long long **total_dev) {
  const int n = (int)ctx->n_nodes;
  const long long ne = ctx->ge_n;
  const int nb = (int)((ne + kSweepBlock - 1) / kSweepBlock);
  RRTX_HIP(ctx, ctx->ws_sweep_mark.ensure((size_t)n));
  RRTX_HIP(ctx, ctx->ws_sweep_flag.ensure((size_t)(ne > 0 ? ne : 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_cnt.ensure(sizeof(int) * (size_t)(nb + 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_start.ensure(sizeof(long long) * (size_t)(nb + 2)));
  hipStream_t st = ctx->stream;
  span_begin(ctx, KF_EDGES);
  hipLaunchKernelGGL(sweep_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ctx->nodes[0], ctx->nodes[1], ctx->nodes[2],
                     n, centre[0], centre[1], centre[2], thr_lt, thr_gt, ctx->ws_sweep_mark.as<uint8_t>());
  if (nb > 0) {
    hipLaunchKernelGGL(sweep_edges_kernel, dim3(nb), dim3(kSweepBlock), 0, st, ctx->ge_start, ctx->ge_end, ne, n,
                       ctx->ws_sweep_mark.as<uint8_t>(), ctx->nodes_aos, ob, active, ctx->ws_sweep_flag.as<uint8_t>(),
                       ctx->ws_sweep_cnt.as<int>());
  }
  launch_excl_scan(st, ctx->ws_sweep_cnt.as<int>(), ctx->ws_sweep_start.as<long long>(), nb);
  if (nb > 0 && cap > 0) {
    hipLaunchKernelGGL(sweep_write_kernel, dim3(nb), dim3(kSweepBlock), 0, st, ctx->ws_sweep_flag.as<uint8_t>(), ne,
                       ctx->ws_sweep_start.as<long long>(), out_dev, (long long)cap);
  }
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  *total_dev = ctx->ws_sweep_start.as<long long>() + nb;
  return RRTX_OK;
}

// device side of rrtx_obstacle_sweep_batch and rrtx_obstacle_release_batch (the mirror is not empty): groups of
// kSweepGroup obstacles in list order, each one mark pass over the nodes, one pass over the mirror, one scan of its
// (obstacle, block) counts and the write of its rows; a group's rows follow the rows of the group before it
// (ws_swb_base[g] = ids before group g).  release: release_edges_words_kernel is the pass over the mirror.  No group
// writes the mirror, so every row sees it as it stood at entry; the caller blocks / unblocks the rows afterwards.
int launch_sphere_burst(rrtx_ctx *ctx, int k, bool release, int32_t *out_dev, int64_t cap, long long **total_dev) {
  const int n = (int)ctx->n_nodes;
  const long long ne = ctx->ge_n;
  const int nb = (int)((ne + kSweepBlock - 1) / kSweepBlock);
  const int ng = (k + kSweepGroup - 1) / kSweepGroup;
  const int kg_max = std::min(k, kSweepGroup);        // (edge ids are int32: kg_max * nb < 2^27 counts, an int for the scan)
  const int na = release ? ctx->sph_view.m : 0;
  if (release && (size_t)na != ctx->rel_stay_host.size()) return fail(ctx, RRTX_E_STATE, "obstacle_release_batch: stay mask of %zu for %d spheres in use", ctx->rel_stay_host.size(), na);
  RRTX_HIP(ctx, ctx->ws_swb_tab.ensure(sizeof(SweepObs) * (size_t)k));
  if (release) RRTX_HIP(ctx, ctx->ws_rel_stay.ensure((size_t)(na > 0 ? na : 1)));
  RRTX_HIP(ctx, ctx->ws_swb_word.ensure(sizeof(unsigned long long) * (size_t)n));
  RRTX_HIP(ctx, ctx->ws_swb_seg_id.ensure(sizeof(int32_t) * (size_t)nb * kSweepBlock));
  RRTX_HIP(ctx, ctx->ws_swb_seg_word.ensure(sizeof(unsigned long long) * (size_t)nb * kSweepBlock));
  RRTX_HIP(ctx, ctx->ws_swb_blk_n.ensure(sizeof(int) * (size_t)nb));
  RRTX_HIP(ctx, ctx->ws_swb_cnt.ensure(sizeof(int) * ((size_t)kg_max * nb + 1)));
  RRTX_HIP(ctx, ctx->ws_swb_pos.ensure(sizeof(long long) * ((size_t)kg_max * nb + 2)));
  RRTX_HIP(ctx, ctx->ws_swb_base.ensure(sizeof(long long) * (size_t)(ng + 1)));
  RRTX_HIP(ctx, ctx->ws_swb_off.ensure(sizeof(int64_t) * (size_t)(k + 1)));
  hipStream_t st = ctx->stream;
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_swb_tab.p, ctx->swb_tab_host.data(), sizeof(SweepObs) * (size_t)k, hipMemcpyHostToDevice, st));
  if (na > 0) RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_rel_stay.p, ctx->rel_stay_host.data(), (size_t)na, hipMemcpyHostToDevice, st));
  RRTX_HIP(ctx, hipMemsetAsync(ctx->ws_swb_base.p, 0, sizeof(long long), st));
  unsigned long long *word = ctx->ws_swb_word.as<unsigned long long>(), *seg_word = ctx->ws_swb_seg_word.as<unsigned long long>();
  int32_t *seg_id = ctx->ws_swb_seg_id.as<int32_t>();
  int *blk_n = ctx->ws_swb_blk_n.as<int>(), *cnt = ctx->ws_swb_cnt.as<int>();
  long long *pos = ctx->ws_swb_pos.as<long long>(), *base = ctx->ws_swb_base.as<long long>();
  span_begin(ctx, KF_EDGES);
  for (int g = 0; g < ng; ++g) {
    const int kg = std::min(kSweepGroup, k - g * kSweepGroup);
    const SweepObs *tab = ctx->ws_swb_tab.as<SweepObs>() + (size_t)g * kSweepGroup;
    hipLaunchKernelGGL(sweep_mark_words_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ctx->nodes[0], ctx->nodes[1],
                       ctx->nodes[2], n, tab, kg, word);
    if (release)
      hipLaunchKernelGGL(release_edges_words_kernel, dim3(nb), dim3(kSweepBlock), 0, st, ctx->ge_dist, ctx->ge_start, ctx->ge_end,
                         ne, n, word, ctx->nodes_aos, tab, kg, nb, ctx->sph_view.rec, ctx->ws_rel_stay.as<uint8_t>(), na,
                         seg_id, seg_word, blk_n, cnt);
    else
      hipLaunchKernelGGL(sweep_edges_words_kernel, dim3(nb), dim3(kSweepBlock), 0, st, ctx->ge_start, ctx->ge_end, ne, n, word,
                         ctx->nodes_aos, tab, kg, nb, seg_id, seg_word, blk_n, cnt);
    launch_excl_scan(st, cnt, pos, kg * nb);
    hipLaunchKernelGGL(sweep_rows_write_kernel, dim3(nb), dim3(kSweepGroup), 0, st, seg_id, seg_word, blk_n, pos, nb, kg, base + g,
                       base + g + 1, ctx->ws_swb_off.as<int64_t>() + (size_t)g * kSweepGroup, out_dev, (long long)cap);
  }
  span_end(ctx);
  RRTX_HIP(ctx, hipGetLastError());
  *total_dev = base + ng;
  return RRTX_OK;
}

// device side of rrtx_obstacle_sweep_polygon_batch: groups of kSweepGroup list entries in the order given.  Per group:
// the word of every node from the group's queries, the candidates (edges that start at a node with a word) compacted
// to (id, word), ONE read of their number, the check of every candidate against the obstacles of its word (Dubins
// space: one steering pass, kernels_dubins.hip), and the sphere burst's tail over the candidates' hit words -- the rows
// follow those of the group before (ws_swb_base).  No group writes the mirror.
// release (rrtx_obstacle_release_polygon_batch): only BLOCKED edges are candidates, and a candidate that collides with an
// obstacle of the stay ranges (ctx->prel_stay_host: pairs [pb, pe) of packed table positions, uploaded once) loses its
// hit word before the tail -- SimpleEdge in the check kernel itself, Dubins in a second kernel over the same steering
// records (kernels_dubins.hip).  The waits are the same: one per group.
int launch_polygon_burst(rrtx_ctx *ctx, int k, double r_min, double robot_radius, bool release, int32_t *out_dev, int64_t cap,
                         long long **total_dev) {
  const char *fn = release ? "obstacle_release_polygon_batch" : "obstacle_sweep_polygon_batch";
  const int n = (int)ctx->n_nodes;
  const long long ne = ctx->ge_n;
  const int nb = (int)((ne + kSweepBlock - 1) / kSweepBlock);
  const int ng = (k + kSweepGroup - 1) / kSweepGroup;
  const int kg_max = std::min(k, kSweepGroup);
  const size_t nq_all = ctx->pswb_q_host.size();
  if ((int)ctx->pswb_qoff_host.size() != ng + 1 || (size_t)ctx->pswb_qoff_host[ng] != nq_all || ctx->pswb_pos_host.size() != (size_t)k)
    return fail(ctx, RRTX_E_STATE, "%s: query tables of %zu groups for %d entries", fn, ctx->pswb_qoff_host.size(), k);
  const int n_stay = release ? (int)(ctx->prel_stay_host.size() / 2) : 0;
  if (release) RRTX_HIP(ctx, ctx->ws_prel_stay.ensure(sizeof(int32_t) * 2 * (size_t)(n_stay > 0 ? n_stay : 1)));
  RRTX_HIP(ctx, ctx->ws_pswb_q.ensure(sizeof(SweepQueryOwned) * (nq_all > 0 ? nq_all : 1)));
  RRTX_HIP(ctx, ctx->ws_pswb_pos.ensure(sizeof(int32_t) * (size_t)k));
  RRTX_HIP(ctx, ctx->ws_pswb_cand_id.ensure(sizeof(int32_t) * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_pswb_cand_word.ensure(sizeof(unsigned long long) * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_pswb_hit.ensure(sizeof(unsigned long long) * (size_t)ne));
  RRTX_HIP(ctx, ctx->ws_sweep_cnt.ensure(sizeof(int) * (size_t)(nb + 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_start.ensure(sizeof(long long) * (size_t)(nb + 2)));
  RRTX_HIP(ctx, ctx->ws_swb_word.ensure(sizeof(unsigned long long) * (size_t)n));
  RRTX_HIP(ctx, ctx->ws_swb_seg_id.ensure(sizeof(int32_t) * (size_t)nb * kSweepBlock));
  RRTX_HIP(ctx, ctx->ws_swb_seg_word.ensure(sizeof(unsigned long long) * (size_t)nb * kSweepBlock));
  RRTX_HIP(ctx, ctx->ws_swb_blk_n.ensure(sizeof(int) * (size_t)nb));
  RRTX_HIP(ctx, ctx->ws_swb_cnt.ensure(sizeof(int) * ((size_t)kg_max * nb + 1)));
  RRTX_HIP(ctx, ctx->ws_swb_pos.ensure(sizeof(long long) * ((size_t)kg_max * nb + 2)));
  RRTX_HIP(ctx, ctx->ws_swb_base.ensure(sizeof(long long) * (size_t)(ng + 1)));
  RRTX_HIP(ctx, ctx->ws_swb_off.ensure(sizeof(int64_t) * (size_t)(k + 1)));
  hipStream_t st = ctx->stream;
  if (nq_all > 0)
    RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_pswb_q.p, ctx->pswb_q_host.data(), sizeof(SweepQueryOwned) * nq_all, hipMemcpyHostToDevice, st));
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_pswb_pos.p, ctx->pswb_pos_host.data(), sizeof(int32_t) * (size_t)k, hipMemcpyHostToDevice, st));
  if (n_stay > 0)
    RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_prel_stay.p, ctx->prel_stay_host.data(), sizeof(int32_t) * 2 * (size_t)n_stay, hipMemcpyHostToDevice, st));
  RRTX_HIP(ctx, hipMemsetAsync(ctx->ws_swb_base.p, 0, sizeof(long long), st));
  const int32_t *stay = release ? ctx->ws_prel_stay.as<int32_t>() : nullptr;
  unsigned long long *word = ctx->ws_swb_word.as<unsigned long long>(), *seg_word = ctx->ws_swb_seg_word.as<unsigned long long>();
  unsigned long long *cand_word = ctx->ws_pswb_cand_word.as<unsigned long long>(), *hit_word = ctx->ws_pswb_hit.as<unsigned long long>();
  int32_t *seg_id = ctx->ws_swb_seg_id.as<int32_t>(), *cand_id = ctx->ws_pswb_cand_id.as<int32_t>();
  int *blk_n = ctx->ws_swb_blk_n.as<int>(), *cnt = ctx->ws_swb_cnt.as<int>();
  long long *pos = ctx->ws_swb_pos.as<long long>(), *base = ctx->ws_swb_base.as<long long>();
  long long *cstart = ctx->ws_sweep_start.as<long long>();
  const bool dubins = ctx->dim == 4;
  int64_t cand_all = 0;
  for (int g = 0; g < ng; ++g) {
    const int kg = std::min(kSweepGroup, k - g * kSweepGroup);
    const int q0 = ctx->pswb_qoff_host[g], nqs = ctx->pswb_qoff_host[g + 1] - q0;
    const int32_t *ppos = ctx->ws_pswb_pos.as<int32_t>() + (size_t)g * kSweepGroup;
    int64_t n_c = 0;
    if (nqs > 0) {                                               // (no query: no obstacle of the group is in use)
      span_begin(ctx, KF_EDGES);
      hipLaunchKernelGGL(sweep_mark_query_words_kernel, dim3((n + 255) / 256), dim3(256), 0, st, ctx->nodes[0], ctx->nodes[1],
                         ctx->nodes[2], ctx->nodes[3], n, ctx->dim, ctx->ws_pswb_q.as<SweepQueryOwned>() + q0, nqs, word);
      hipLaunchKernelGGL((release ? sweep_cand_count_kernel<true> : sweep_cand_count_kernel<false>), dim3(nb), dim3(kSweepBlock), 0,
                         st, ctx->ge_start, ne, n, word, ctx->ge_dist, ctx->ws_sweep_cnt.as<int>());
      launch_excl_scan(st, ctx->ws_sweep_cnt.as<int>(), cstart, nb);
      hipLaunchKernelGGL((release ? sweep_cand_write_kernel<true> : sweep_cand_write_kernel<false>), dim3(nb), dim3(kSweepBlock), 0,
                         st, ctx->ge_start, ne, n, word, ctx->ge_dist, cstart, cand_id, cand_word);
      span_end(ctx);
      RRTX_HIP(ctx, hipGetLastError());
      RRTX_HIP(ctx, hipMemcpyAsync(&n_c, cstart + nb, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      RRTX_HIP(ctx, hipStreamSynchronize(st));                   // the group's one wait: the count sizes the check launch
      if (n_c < 0 || n_c > ne) return fail(ctx, RRTX_E_DEVICE, "%s: %lld candidates of %lld edges", fn, (long long)n_c, ne);
    }
    cand_all += n_c;
    if (n_c > 0) {
      if (dubins) {
        const int rc = launch_dubins_check_words(ctx, cand_id, cand_word, n_c, r_min, robot_radius, ppos, kg, hit_word, stay, n_stay);
        if (rc) return rc;
      } else {
        const PolyView &V = ctx->poly_view;
        span_begin(ctx, KF_EDGES);
        const dim3 grid((unsigned)((n_c + 255) / 256));
        if (release)
          hipLaunchKernelGGL(release_polygon_words_kernel, grid, dim3(256), 0, st, cand_id, cand_word, (long long)n_c, ctx->ge_start,
                             ctx->ge_end, n, ctx->nodes_aos, V.meta, V.off, V.vxy, V.path_off, V.path, ppos, robot_radius, hit_word, stay,
                             n_stay, V.m);
        else
          hipLaunchKernelGGL(sweep_polygon_words_kernel, grid, dim3(256), 0, st, cand_id, cand_word, (long long)n_c, ctx->ge_start,
                             ctx->ge_end, n, ctx->nodes_aos, V.meta, V.off, V.vxy, V.path_off, V.path, ppos, robot_radius, hit_word);
        span_end(ctx);
      }
    }
    // (a group without candidates still writes its kg empty rows: one block over no candidate)
    const int nbc = n_c > 0 ? (int)((n_c + kSweepBlock - 1) / kSweepBlock) : 1;
    span_begin(ctx, KF_EDGES);
    hipLaunchKernelGGL(sweep_cand_rows_kernel, dim3(nbc), dim3(kSweepBlock), 0, st, cand_id, hit_word, (long long)n_c, kg, nbc,
                       seg_id, seg_word, blk_n, cnt);
    launch_excl_scan(st, cnt, pos, kg * nbc);
    hipLaunchKernelGGL(sweep_rows_write_kernel, dim3(nbc), dim3(kSweepGroup), 0, st, seg_id, seg_word, blk_n, pos, nbc, kg, base + g,
                       base + g + 1, ctx->ws_swb_off.as<int64_t>() + (size_t)g * kSweepGroup, out_dev, (long long)cap);
    span_end(ctx);
    RRTX_HIP(ctx, hipGetLastError());
  }
  ctx->last_sweep_candidates = cand_all;
  *total_dev = base + ng;
  return RRTX_OK;
}

// ---- the polygon / Dubins sweep: compaction steps shared by rrtx_obstacle_sweep_polygon (rrtx_capi.hip) ----
int launch_sweep_mark_multi(rrtx_ctx *ctx, const SweepQuery *queries_host, int nqs) {
  const int n = (int)ctx->n_nodes;
  RRTX_HIP(ctx, ctx->ws_sweep_mark.ensure((size_t)n));
  RRTX_HIP(ctx, ctx->ws_mask.ensure(sizeof(SweepQuery) * (size_t)nqs));
  RRTX_HIP(ctx, hipMemcpyAsync(ctx->ws_mask.p, queries_host, sizeof(SweepQuery) * (size_t)nqs, hipMemcpyHostToDevice, ctx->stream));
  RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));          // (the caller's table is a local)
  hipLaunchKernelGGL(sweep_mark_multi_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->nodes[0], ctx->nodes[1],
                     ctx->nodes[2], ctx->nodes[3], n, ctx->dim, ctx->ws_mask.as<SweepQuery>(), nqs, ctx->ws_sweep_mark.as<uint8_t>());
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

// positions with flag != 0 -> out (ids[position] when ids is given), ascending; *total_dev = their number
static int compact_flags(rrtx_ctx *ctx, long long n, const int32_t *ids_dev, int32_t *out_dev, long long cap, long long **total_dev) {
  const int nb = (int)((n + kSweepBlock - 1) / kSweepBlock);
  launch_excl_scan(ctx->stream, ctx->ws_sweep_cnt.as<int>(), ctx->ws_sweep_start.as<long long>(), nb);
  if (nb > 0 && cap > 0)
    hipLaunchKernelGGL(sweep_write_kernel, dim3(nb), dim3(kSweepBlock), 0, ctx->stream, ctx->ws_sweep_flag.as<uint8_t>(), n,
                       ctx->ws_sweep_start.as<long long>(), out_dev, cap, ids_dev);
  RRTX_HIP(ctx, hipGetLastError());
  *total_dev = ctx->ws_sweep_start.as<long long>() + nb;
  return RRTX_OK;
}

// mirrored edges that start at a marked node (blocked_only: and have dist == Inf) -> ascending ids in out_dev
int launch_sweep_select(rrtx_ctx *ctx, int blocked_only, int32_t *out_dev, long long cap, long long **total_dev) {
  const long long ne = ctx->ge_n;
  const int nb = (int)((ne + kSweepBlock - 1) / kSweepBlock);
  RRTX_HIP(ctx, ctx->ws_sweep_flag.ensure((size_t)(ne > 0 ? ne : 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_cnt.ensure(sizeof(int) * (size_t)(nb + 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_start.ensure(sizeof(long long) * (size_t)(nb + 2)));
  if (nb > 0)
    hipLaunchKernelGGL(sweep_select_kernel, dim3(nb), dim3(kSweepBlock), 0, ctx->stream, ctx->ge_start, ne, (int)ctx->n_nodes,
                       ctx->ws_sweep_mark.as<uint8_t>(), ctx->ge_dist, blocked_only, ctx->ws_sweep_flag.as<uint8_t>(),
                       ctx->ws_sweep_cnt.as<int>());
  return compact_flags(ctx, ne, nullptr, out_dev, cap, total_dev);
}

// of the n candidates ids_dev[k]: those with hit[k] and neither o1[k] nor o2[k] -> their ids, ascending
int launch_sweep_finish(rrtx_ctx *ctx, const int32_t *ids_dev, long long n, const uint8_t *hit, const uint8_t *o1,
                        const uint8_t *o2, int32_t *out_dev, long long cap, long long **total_dev) {
  const int nb = (int)((n + kSweepBlock - 1) / kSweepBlock);
  RRTX_HIP(ctx, ctx->ws_sweep_flag.ensure((size_t)(n > 0 ? n : 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_cnt.ensure(sizeof(int) * (size_t)(nb + 1)));
  RRTX_HIP(ctx, ctx->ws_sweep_start.ensure(sizeof(long long) * (size_t)(nb + 2)));
  if (nb > 0)
    hipLaunchKernelGGL(sweep_combine_kernel, dim3(nb), dim3(kSweepBlock), 0, ctx->stream, hit, o1, o2, n,
                       ctx->ws_sweep_flag.as<uint8_t>(), ctx->ws_sweep_cnt.as<int>());
  return compact_flags(ctx, n, ids_dev, out_dev, cap, total_dev);
}

int launch_sweep_gather(rrtx_ctx *ctx, const int32_t *ids_dev, long long n, double *p0_dev, double *p1_dev) {
  if (n <= 0) return RRTX_OK;
  hipLaunchKernelGGL(sweep_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ids_dev, n, ctx->ge_start,
                     ctx->ge_end, ctx->nodes_aos, ctx->dim, p0_dev, p1_dev);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

}  // namespace rrtx
