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
// Samples of one batch do not see each other -- the lists are against the tree as it stood, exactly as in
// rrtx_extend_candidates -- so a node may appear in the rewire lists of several samples; settling that is the
// caller's bookkeeping.
//
// Layout.  Segments average ~25 entries at C4 size and range from 0 to a few hundred: a wave per sample would idle
// most lanes, a lane per sample would serialise the long lists.  Samples are dealt to sub-wave GROUPS of 8, 16, 32
// or 64 lanes -- the smallest power of two that covers the mean segment length, which every wave reads off
// offsets[nq] -- and a group strides over its segment, so the reads of one group are contiguous.
//   select_parent_kernel  every lane keeps the (value, position) of the first minimum among its own entries
//                         (ascending positions, strict >), the group reduces the pairs lexicographically by
//                         butterfly exchange: the winner is the lowest position by construction, no atomics.  A second
//                         walk counts the sample's rewire entries.
//   select_scan_kernel    one workgroup: exclusive scan of the per-sample counts -> rw_offsets, rw_needed.
//   select_rewire_kernel  the same walk again; a ballot over the group's lanes gives every reported entry its place
//                         behind rw_offsets[s], in list order.  Entries at or beyond rw_cap are not written.
// The sample loop is wave-uniform (groups past the last sample walk an empty segment), so the exchanges after it run
// with every lane active; inside the entry loop only ballots are used, which count active lanes only.
// Every index is checked before it is used: list positions against cap, node indices against the length of lmc.
#include "rrtx_internal.hpp"

namespace rrtx {
namespace {

constexpr int kSelBlock = 256;
constexpr int kSelWave = 64;

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

// lanes per sample: the smallest of 8, 16, 32, 64 that covers the mean segment length
__device__ __forceinline__ int sel_group(const SelArgs &a) {
  long long total = a.offsets[a.nq];
  if (total < 0) total = 0;
  const long long mean = total / (a.nq > 0 ? a.nq : 1);
  int g = 8;
  while (g < kSelWave && g < mean) g <<= 1;
  return g;
}

// the segment of sample s, clipped to what the arrays hold
__device__ __forceinline__ void sel_segment(const SelArgs &a, long long s, long long &beg, long long &end) {
  beg = 0; end = 0;
  if (s >= a.nq) return;
  long long b = a.offsets[s], e = a.offsets[s + 1];
  if (e > a.cap) e = a.cap;
  if (b < 0 || b > e) return;
  beg = b; end = e;
}

__device__ __forceinline__ double sel_lmc(const SelArgs &a, int j) {
  return ((unsigned long long)(long long)j < (unsigned long long)a.n_lmc) ? a.lmc[j] : __builtin_huge_val();
}

__global__ __launch_bounds__(kSelBlock) void select_parent_kernel(SelArgs a) {
  if (sel_overflow(a)) {
    for (long long s = (long long)blockIdx.x * kSelBlock + threadIdx.x; s < a.nq; s += (long long)gridDim.x * kSelBlock)
      a.status[s] = RRTX_SEL_OVERFLOW;
    return;
  }
  const int g = sel_group(a);
  const int lane = threadIdx.x & (kSelWave - 1);
  const int sub = lane & (g - 1);
  const long long stride = (long long)gridDim.x * kSelBlock / g;
  for (long long s0 = ((long long)blockIdx.x * kSelBlock + (threadIdx.x - lane)) / g; s0 < a.nq; s0 += stride) {
    const long long s = s0 + lane / g;
    long long beg, end;
    sel_segment(a, s, beg, end);
    const bool live = s < a.nq;
    const bool unsafe = live && a.unsafe && a.unsafe[s] != 0;
    if (unsafe) end = beg;
    double best = __builtin_huge_val();
    int pos = 0x7fffffff;
    for (long long e = beg + sub; e < end; e += g) {
      if (a.hit_out[e] != 0) continue;
      const double cand = sel_lmc(a, a.idx[e]) + a.cost_out[e];
      if (best > cand) { best = cand; pos = (int)(e - beg); }
    }
    for (int off = g >> 1; off > 0; off >>= 1) {
      const double ov = __shfl_xor(best, off);
      const int op = __shfl_xor(pos, off);
      if (ov < best || (ov == best && op < pos)) { best = ov; pos = op; }
    }
    const bool ok = pos != 0x7fffffff;
    const int parent = ok ? a.idx[beg + pos] : -1;
    int cnt = 0;
    if (ok)
      for (long long e = beg + sub; e < end; e += g) {
        if (a.hit_in[e] != 0) continue;
        const int j = a.idx[e];
        if (j == parent) continue;
        if (sel_lmc(a, j) > best + a.cost_in[e]) ++cnt;
      }
    for (int off = g >> 1; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (live && sub == 0) {
      a.status[s] = unsafe ? RRTX_SEL_UNSAFE : (beg == end ? RRTX_SEL_EMPTY : (ok ? RRTX_SEL_OK : RRTX_SEL_NO_PARENT));
      a.parent_idx[s] = parent;
      a.parent_entry[s] = ok ? beg + pos : -1;
      a.lmc_new[s] = best;
      a.rw_count[s] = cnt;
    }
  }
}

// exclusive scan of the per-sample counts by one workgroup, 4096 samples per round: a thread takes four consecutive
// counts (one 16-byte load, so a wave reads 1 KB in a row), the waves scan their sums, the round's total is carried on
__global__ __launch_bounds__(1024) void select_scan_kernel(SelArgs a) {
  if (sel_overflow(a)) return;
  __shared__ long long wave_sum[16];
  const int t = threadIdx.x, lane = t & (kSelWave - 1), w = t / kSelWave;
  long long carry = 0;
  for (long long base = 0; base < a.nq; base += 4096) {
    const long long i0 = base + 4 * (long long)t;
    int c[4] = {0, 0, 0, 0};
    if (i0 + 3 < a.nq) {
      const int4 v = *reinterpret_cast<const int4 *>(a.rw_count + i0);
      c[0] = v.x; c[1] = v.y; c[2] = v.z; c[3] = v.w;
    } else {
      for (int k = 0; k < 4; ++k)
        if (i0 + k < a.nq) c[k] = a.rw_count[i0 + k];
    }
    const long long local = (long long)c[0] + c[1] + c[2] + c[3];
    long long incl = local;
    for (int off = 1; off < kSelWave; off <<= 1) {
      const long long o = __shfl_up(incl, off);
      if (lane >= off) incl += o;
    }
    if (lane == kSelWave - 1) wave_sum[w] = incl;
    __syncthreads();
    long long before = carry, round_total = 0;
    for (int k = 0; k < 16; ++k) {
      if (k < w) before += wave_sum[k];
      round_total += wave_sum[k];
    }
    long long run = before + incl - local;
    for (int k = 0; k < 4; ++k)
      if (i0 + k < a.nq) { a.rw_offsets[i0 + k] = run; run += c[k]; }
    carry += round_total;
    __syncthreads();
  }
  if (t == 0) { a.rw_offsets[a.nq] = carry; *a.rw_needed = carry; }
}

__global__ __launch_bounds__(kSelBlock) void select_rewire_kernel(SelArgs a) {
  if (sel_overflow(a)) return;
  const int g = sel_group(a);
  const int lane = threadIdx.x & (kSelWave - 1);
  const int sub = lane & (g - 1);
  const unsigned long long group_mask = (g == kSelWave ? ~0ull : ((1ull << g) - 1ull)) << (lane - sub);
  const unsigned long long below = group_mask & ((1ull << lane) - 1ull);
  const long long stride = (long long)gridDim.x * kSelBlock / g;
  for (long long s0 = ((long long)blockIdx.x * kSelBlock + (threadIdx.x - lane)) / g; s0 < a.nq; s0 += stride) {
    const long long s = s0 + lane / g;
    if (s >= a.nq || a.status[s] != RRTX_SEL_OK) continue;
    long long beg, end;
    sel_segment(a, s, beg, end);
    const double best = a.lmc_new[s];
    const int parent = a.parent_idx[s];
    long long at = a.rw_offsets[s];
    for (long long e0 = beg; e0 < end; e0 += g) {
      const long long e = e0 + sub;
      bool take = false;
      int j = -1;
      double v = 0.0;
      if (e < end && a.hit_in[e] == 0) {
        j = a.idx[e];
        v = best + a.cost_in[e];
        take = j != parent && sel_lmc(a, j) > v;
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
  a.offsets = L.offsets; a.idx = L.idx; a.cost_out = L.cost_out; a.cost_in = L.cost_in;
  a.hit_out = L.hit_out; a.hit_in = L.hit_in;
  a.n_valid = L.n_valid_dev; a.cap = (long long)L.cap;
  a.unsafe = L.sample_unsafe; a.lmc = L.lmc; a.n_lmc = (long long)L.n_lmc;
  a.parent_idx = L.parent_idx; a.parent_entry = L.parent_entry; a.lmc_new = L.lmc_new; a.status = L.status;
  a.rw_count = ctx->ws_sel_cnt.as<int>();
  a.rw_offsets = L.rw_offsets; a.rw_node = L.rw_node; a.rw_value = L.rw_value; a.rw_cap = (long long)L.rw_cap;
  a.rw_needed = L.rw_needed_dev;
  // a group of 32 lanes per sample fills the device once (8 waves on each of 1024 SIMDs); beyond that the groups stride
  long long blocks = ((long long)L.nq * 32 + kSelBlock - 1) / kSelBlock;
  blocks = std::max(1ll, std::min(blocks, 2048ll));
  if (L.nq > 0) hipLaunchKernelGGL(select_parent_kernel, dim3((unsigned)blocks), dim3(kSelBlock), 0, ctx->stream, a);
  hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, a);
  if (L.nq > 0) hipLaunchKernelGGL(select_rewire_kernel, dim3((unsigned)blocks), dim3(kSelBlock), 0, ctx->stream, a);
  RRTX_HIP(ctx, hipGetLastError());
  return RRTX_OK;
}

// the context's own rrtLMC array: one fp64 per node, +Inf until set
int node_cost_ensure(rrtx_ctx *ctx) {
  const int64_t n = ctx->n_nodes;
  if (n > ctx->node_lmc_cap || !ctx->node_lmc) {
    const int64_t nc = std::max<int64_t>(std::max<int64_t>(ctx->cap_nodes, n), 1024);
    double *nb = nullptr;
    hipError_t e = hipMalloc(&nb, sizeof(double) * (size_t)nc);
    if (e != hipSuccess) return fail(ctx, RRTX_E_NOMEM, "hipMalloc of %lld node costs failed: %s", (long long)nc, hipGetErrorString(e));
    if (ctx->node_lmc) {
      if (ctx->node_lmc_n > 0)
        RRTX_HIP(ctx, hipMemcpyAsync(nb, ctx->node_lmc, sizeof(double) * (size_t)ctx->node_lmc_n, hipMemcpyDeviceToDevice, ctx->stream));
      RRTX_HIP(ctx, hipStreamSynchronize(ctx->stream));
      RRTX_HIP(ctx, hipFree(ctx->node_lmc));
    }
    ctx->node_lmc = nb;
    ctx->node_lmc_cap = nc;
  }
  if (n > ctx->node_lmc_n) {
    const long long m = (long long)(n - ctx->node_lmc_n);
    hipLaunchKernelGGL(select_fill_inf_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, ctx->node_lmc,
                       (long long)ctx->node_lmc_n, m);
    RRTX_HIP(ctx, hipGetLastError());
    ctx->node_lmc_n = n;
  }
  return RRTX_OK;
}

}  // namespace rrtx
