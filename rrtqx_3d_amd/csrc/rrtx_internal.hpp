// rrtx_internal.hpp -- context, device buffers and launch declarations shared by
// the HIP translation units of librrtx_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rrtx.h"

namespace rrtx {

constexpr int kMaxWraps = 3;
constexpr int kMaxSlots = 1 << kMaxWraps;  // query copies per query (original + ghosts)

// ---- records shared between host and device --------------------------------
// One query copy as the scan kernel reads it with scalar loads.
struct alignas(32) QRec3 { double x, y, z, thr; };                 // thr: hit <=> d2 < thr
struct alignas(64) QRec4 { double x, y, z, w, thr, pad0, pad1, pad2; };
template <int D> struct QRecT;
template <> struct QRecT<3> { using type = QRec3; };
template <> struct QRecT<4> { using type = QRec4; };

// Fixed-slot table entry: slot j of query i lives at [i * n_slots + j].  Slot 0 is
// the query itself, slots 1.. are its ghosts in the reference's iterator order
// (R/ghostPoint.jl:60-111).  thr_lt < 0 marks a ghost the iterator skips.
struct alignas(64) SlotRec { double x, y, z, w, thr_lt, thr_gt, pad0, pad1; };

// One range-search hit: node `idx` is within range of query `owner`; d2 is the
// squared distance to the copy that discovered it first.
struct alignas(16) HitRec { int32_t owner; int32_t idx; double d2; };

// Active sphere as the edge kernel reads it: centre + threshold on the squared
// distance (hit <=> !(s >= thr), thr = first s with sqrt(s) > robotRadius+radius).
struct alignas(32) SphRec { double cx, cy, cz, thr; };

// One obstacle of a batched sweep (rrtx_obstacle_sweep_batch) as its two kernels read it: the SphRec of the edge test
// (its centre is also the centre of the range query), the two thresholds of the range query on the squared distance
// (node in range <=> s < thr_lt, the root: s < thr_gt) and whether the obstacle is in use.
struct alignas(64) SweepObs { SphRec ob; double thr_lt, thr_gt; int32_t active, pad0; double pad1; };

// One range query of the polygon / Dubins sweep as sweep_mark_multi_kernel reads it (kernels_sweep.hip): node in range
// <=> s < thr_lt, the root: s < thr_root
struct SweepQuery { double x, y, z, w, thr_lt, thr_root; };

// A range query of the batched polygon sweep (rrtx_obstacle_sweep_polygon_batch) as sweep_mark_query_words_kernel reads
// it: the query, and the bit of the group's word that stands for the obstacle the query belongs to
struct alignas(64) SweepQueryOwned { SweepQuery q; unsigned long long owner; double pad; };

// host-side mirror of exact_math.hpp's ChunkExt (this header is also read by plain C++)
struct ChunkExtHost { unsigned long long xlo, xhi, ylo, yhi; };

// ---- owners of device and pinned memory --------------------------------------
// Every allocation of the library belongs to a member of one of these types and is released by its destructor; they
// move and do not copy.  hipMalloc / hipFree / hipHostMalloc / hipHostFree are called here and nowhere else.
template <hipError_t (*Free)(void *)>
struct Owned {
  void *p = nullptr;
  size_t bytes = 0;
  Owned() = default;
  Owned(const Owned &) = delete;   // (and so no copy assignment either: a move assignment is declared)
  Owned(Owned &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
  Owned &operator=(Owned &&o) noexcept {   // (releases what it held)
    if (this != &o) { release(); std::swap(p, o.p); std::swap(bytes, o.bytes); }
    return *this;
  }
  ~Owned() { release(); }
  void release() { if (p) (void)Free(p); p = nullptr; bytes = 0; }
  template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
struct DevBuf : Owned<hipFree> {
  size_t grown(size_t need) const {   // what a need beyond `bytes` is rounded to: doubled from 4096 or from what is held
    size_t nb = bytes ? bytes : 4096;
    while (nb < need) nb *= 2;
    return nb;
  }
  hipError_t ensure(size_t need) {     // room for `need` bytes; what the buffer held is not kept
    if (need <= bytes) return hipSuccess;
    const size_t nb = grown(need);
    if (p) { hipError_t e = hipFree(p); if (e != hipSuccess) return e; p = nullptr; bytes = 0; }
    hipError_t e = hipMalloc(&p, nb);
    if (e == hipSuccess) bytes = nb;
    return e;
  }
  // THE grow-and-keep routine: a new block of exactly `new_bytes`, the first `keep` bytes of the old one copied on `st`
  // and waited for, the old block freed.  On failure the new block is freed and the old one stays.
  hipError_t regrow(size_t new_bytes, size_t keep, hipStream_t st) {
    DevBuf nb;
    hipError_t e = hipMalloc(&nb.p, new_bytes);
    if (e != hipSuccess) return e;
    nb.bytes = new_bytes;
    if (p && keep > 0) e = hipMemcpyAsync(nb.p, p, keep, hipMemcpyDeviceToDevice, st);
    if (p && e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) *this = std::move(nb);
    return e;
  }
  hipError_t ensure_keep(size_t need, size_t keep, hipStream_t st) {   // ensure, keeping the first `keep` bytes
    return need <= bytes ? hipSuccess : regrow(grown(need), keep, st);
  }
};
// A device array of T, read where a T * is expected and sized by its owner's policy (regrow: exactly `count` elements).
// get() is for the places an implicit conversion does not reach: a deduced template parameter, a cast.
template <class T>
struct DevArray {
  DevBuf buf;
  T *get() const { return buf.as<T>(); }
  operator T *() const { return get(); }
  hipError_t regrow(size_t count, size_t keep, hipStream_t st) { return buf.regrow(sizeof(T) * count, sizeof(T) * keep, st); }
};
// pinned host memory (hipHostMalloc with the given flags); alloc replaces what is held
struct PinnedBuf : Owned<hipHostFree> {
  hipError_t alloc(size_t nb, unsigned flags) {
    release();
    const hipError_t e = hipHostMalloc(&p, nb, flags);
    if (e == hipSuccess) bytes = nb;
    return e;
  }
};
static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_constructible<DevArray<double>>::value &&
              !std::is_copy_constructible<PinnedBuf>::value, "an allocation has one owner");

// a node without a parent edge in GraphCost::parent (the root, an orphan); and what rrtx_graph_edges_compact leaves in
// GraphCost::rep_parent for a parent edge it removed: neither -1 (none) nor an edge id, so the next delta reports the node
constexpr int32_t kNoParentEdge = 0x7fffffff;
constexpr int32_t kRemovedEdge = -2;

// cost propagation over the edge mirror (kernels_graph.hip): the state of the last solve stays on the device
struct GraphCost {
  DevBuf lmc, parent, stamp, flags, orph, anc, ids;
  DevBuf in_cnt, in_start, in_cursor, in_tiles;     // CSR of in-edges: per end node, ...
  DevBuf in_src, in_w, in_pos;                      // ... start node and cost of every in-edge; slot of every edge id
  int64_t in_ne = 0;                                // edges the CSR holds ([in_ne, ge_n) is the tail)
  int in_nn = 0;                                    // nodes the CSR holds
  int solved_root = -1;
  int64_t solved_nodes = 0, solved_edges = 0;
  bool touched_old = false;                         // set_dist / block since the last solve
  // what rrtx_graph_cost_update_delta last reported: per node the bit pattern of rrtLMC and the parent edge (-1: none)
  DevBuf rep_lmc, rep_parent;
  int rep_root = -1;                                // -1: nothing reported
  int64_t rep_nodes = 0;                            // nodes the two arrays are initialised for (beyond: +Inf / -1)
  DevBuf delta_cnt, delta_pos;                      // differing nodes per workgroup, their exclusive scan
};

// ---- the packed obstacle tables on the device, as the launch sites read them ---------
// One view per list: const device pointers into the list's one block (SphereTableBlock / PolygonTableBlock,
// block_layout.hpp) and its counts.  sync_spheres / sync_polygons rewrite the context's view at their end, after the
// block's ensure (the invariant of Lists below).  Nothing in use: m = 0 and null pointers, whatever the buffer holds.
struct SphView {
  const SphRec *rec = nullptr, *reach = nullptr;   // exact records; centre + inflated reach (conservative skip test)
  const float *reach_f = nullptr;                  // fp32, origin-relative, pair-interleaved groups of 8 (the packed screen)
  const double *sample = nullptr;                  // SampleSph (collide_device.hpp) by its scalars, 8 a sphere
  const double *radius = nullptr, *thr_in = nullptr;
  const int32_t *orig = nullptr;                   // list position of every packed sphere
  int m = 0;                                       // spheres in use
};
struct PolyView {
  const double *meta = nullptr;                    // per obstacle in use {cx, cy, radius, kind}
  const int32_t *off = nullptr;                    // vertex CSR
  const double *vxy = nullptr, *vslope = nullptr;  // per vertex v: slope of the side that ends at v (R/DRRT.jl:1178)
  const int32_t *orig = nullptr;                   // list position of every packed obstacle
  // the exact box of the obstacle's vertices (xmin, xmax, ymin, ymax); the box of its centre over its whole path
  // (kinds 6 / 7; a point otherwise); the sorted y of every vertex of the kind-3 polygons (n_ytab < 0: no table)
  const double *bbox = nullptr, *pbox = nullptr, *ytab = nullptr;
  int n_ytab = 0;
  const int32_t *path_off = nullptr;               // kinds 6 / 7: rows of (dx, dy, t), CSR over the packed obstacles
  const double *path = nullptr;
  int m = 0;                                       // obstacles in use
  bool has_moving = false;                         // one of them is of kind 6 or 7
};

enum KernelFamily { KF_NN_SCAN = 0, KF_NN_FINISH, KF_NN_NEAREST, KF_EDGES, KF_POINTS, KF_DUBINS, KF_DUBINS_STEER, KF_COUNT };

struct TimedSpan { hipEvent_t a, b; int family; };

}  // namespace rrtx

struct rrtx_ctx {
  int dim = 3;
  int device = 0;
  hipStream_t own_stream = nullptr;
  // host-pointer entry points: results leave the device through ONE pinned staging arena (hipHostMalloc; DMA at PCIe
  // rate, no driver-side staging of pageable memory) and are copied into the caller's arrays after the final sync --
  // unless the caller registered its arrays (rrtx_host_register), in which case the DMA goes straight to them
  rrtx::PinnedBuf h_arena;
  size_t h_arena_used = 0;
  struct HostCopy { void *dst; const void *src; size_t bytes; };
  std::vector<HostCopy> h_pending;                       // arena -> caller copies to run after the next sync
  std::vector<std::pair<const char *, size_t>> h_registered;
  hipStream_t stream = nullptr;
  std::string err;

  // node SoA (fp64), one array per coordinate
  rrtx::DevArray<double> nodes[4];
  // the same coordinates, four doubles per node (x y z w): one 32-byte read per random node access
  rrtx::DevArray<double> nodes_aos;
  // fp32 shadow of the node SoA for the conservative range prefilter
  // (kernels_nn.hip, nn_scan_f32_kernel); never used to decide a result
  rrtx::DevArray<float> nodes_f[4];
  rrtx::DevArray<float> nodes_pp;   // |p~|^2 of the shifted fp32 coordinates
  double origin[4] = {0, 0, 0, 0};  // shift applied before the fp32 conversion (first node)
  bool origin_set = false;
  int64_t n_nodes = 0, cap_nodes = 0;
  rrtx::DevBuf d_absmax;            // uint64: bit pattern of max |coordinate| over all nodes

  // Slab-ordered copy of the fp32 shadow for the culled range scan (kernels_nn.hip, "slab
  // index").  Positions [0, sl_n_sorted) hold nodes 0..sl_n_sorted-1 ordered by equal-width
  // (x, y) grid cell and, inside a cell, by bin of the third coordinate (sl_kz bins); positions
  // >= sl_n_sorted hold node p at position p (appended since the last rebuild; a batch appended
  // as a sorted run is in cell order inside its own range of positions).  chunk_ext: exact fp64 x and y extent of every 512-position chunk (enc_ord).
  // Inside a chunk the positions are lane-major: scan lane L owns positions 8 L .. 8 L + 7, so
  // its eight nodes are two 16-byte loads per array and the exact re-test of a flagged lane
  // reads eight consecutive doubles (sl_d: the same order in fp64).
  rrtx::DevArray<float> sl_f[4];
  rrtx::DevArray<double> sl_d[4];
  rrtx::DevArray<float> sl_pp;
  rrtx::DevArray<int32_t> sl_id;
  rrtx::DevArray<rrtx::ChunkExtHost> chunk_ext;   // x / y extent of every chunk (enc_ord), see exact_math.hpp ChunkExt
  int64_t cap_chunks = 0;
  int64_t sl_n_sorted = 0;
  double sl_run_chunks = 0.0;       // chunks of the tail that were appended as sorted runs
  int sl_cells = 0;                 // cells of the grid of the last rebuild
  int sl_kz = 0;                    // bins of the third coordinate inside a cell (0: no index yet)
  double sl_debt_us = 0.0;          // what the appended tail has cost the searches since the last rebuild (estimate)
  rrtx::DevBuf d_xrange;            // uint64[6]: enc_ord of min / max node x, min / max node y, min / max of the third coordinate
  rrtx::DevBuf ws_slab_hist, ws_slab_start, ws_slab_sr, ws_slab_params, ws_run_hist, ws_run_sr;
  int run_hist_flip = 0;            // the sorted runs alternate between two cell histograms (each run's place kernel clears the other)

  // options (rrtx_set_option)
  int opt_nn_filter = 1;            // 1: fp32 prefilter + exact fp64 confirm, 0: exact fp64 scan
  int opt_scan_blocks = 1280;       // persistent workgroups of the range scan (256 CUs x 5 resident)
  int opt_scan_items = 2048;        // target number of (tile, segment) work items
  int opt_tile_q = 0;               // query copies per workgroup tile (0 = kernel default)
  int opt_nn_cull = 1;              // 0 off, 1 auto (trees of >= 8192 nodes), 2 always
  long long opt_nearest_rec_cap = 0; // testing: candidate record capacity of the screened nearest scan (0 = default)
  int opt_space_has_time = 0;       // CSpace.spaceHasTime for the Dubins entry points ([x y t theta], R/DRRT_data_structures.jl:330)
  int opt_dubins_time_column = 0;   // RRTX_OPT_DUBINS_TIME_COLUMN: 0 the kernels' piecewise form, 1 the reference's running sum
  double dubins_vmin = 0.0, dubins_vmax = 1e300;   // S.dubinsMinVelocity / dubinsMaxVelocity (validMove)
  int opt_root_rule = 1;            // 0: node 0 is not the tree's root (this context holds a later node range)
  int opt_tune = 0;                 // experiment switches (RRTX_OPT_TUNE), never change a result
  int opt_profile_every = 1;        // profiling level 1 times every n-th launch of the search kernel
  long long span_tick = 0;

  // wrapped dimensions
  int n_wraps = 0;
  int wrap_dim[rrtx::kMaxWraps] = {0, 0, 0};
  double wrap_period[rrtx::kMaxWraps] = {0, 0, 0};

  // sphere obstacles: host truth (list order) + packed active device copy
  std::vector<double> sph;          // m x 4
  std::vector<uint8_t> sph_active;  // m
  bool sph_dirty = true;
  double sph_packed_rr = -1.0;      // robot radius the packed thresholds were built for
  rrtx::DevBuf d_sph_tab;           // SphereTableBlock (block_layout.hpp): the packed tables, one allocation and one upload
  rrtx::SphView sph_view;           // ... as the launch sites read them; rewritten by every sync_spheres
  double sph_packed_origin[3] = {0, 0, 0};   // origin the fp32 reach groups are relative to
  // polygon obstacles
  std::vector<int32_t> poly_off;    // m+1
  std::vector<double> poly_vxy;
  std::vector<double> poly_cr;      // m x 3
  std::vector<uint8_t> poly_kind, poly_active;
  bool poly_dirty = true;
  rrtx::DevBuf d_poly_tab;          // PolygonTableBlock (block_layout.hpp): the packed tables, one allocation and one upload
  rrtx::PolyView poly_view;         // ... as the launch sites read them; rewritten by every sync_polygons
  // uniform grid over the packed obstacles for the flag-only point check (sync_polygon_grid, PolygonGridBlock): per cell
  rrtx::DevBuf d_poly_grid;         // the obstacles whose bounding circle or box, padded by poly_grid_pad, reaches the cell
  std::vector<double> poly_h_meta, poly_h_bbox;      // host copies of the packed records the grid is built from
  double poly_grid_pad = -1.0;                        // < 0: no grid
  double poly_grid_x0 = 0.0, poly_grid_y0 = 0.0, poly_grid_inv_wx = 0.0, poly_grid_inv_wy = 0.0;
  int poly_grid_g = 0;
  rrtx::DevBuf ws_knn_off, ws_knn_idx, ws_knn_dist, ws_knn_misc;   // k-nearest via range-search lists
  int opt_knn_lists = 1;
  int opt_extend_polygons = 0;   // rrtx_extend_candidates checks against the polygon list instead of the spheres
  // kinds 6 / 7 (polygons moving in time): per obstacle rows of (dx, dy, t), CSR over all m obstacles
  std::vector<int32_t> poly_path_off;
  std::vector<double> poly_path;

  // workspaces
  rrtx::DevBuf ws_q;        // staged queries / points
  rrtx::DevBuf ws_q2;
  rrtx::DevBuf ws_slots;    // SlotRec table
  rrtx::DevBuf ws_copies;   // QRec copies
  rrtx::DevBuf ws_copies_f; // fp32 prefilter copies
  rrtx::DevBuf ws_copy_meta;// int32 owner, slot per copy
  rrtx::DevBuf ws_copies_s, ws_meta_s;  // copies / meta in bucket order (culled scan)
  rrtx::DevBuf ws_cb, ws_qhist;         // (bucket, rank) per copy; bucket histogram
  rrtx::DevBuf ws_qslot;                // bucket-slot table of the culled search without ghosts (QSlots)
  rrtx::DevBuf ws_bkt;      // per-query hit buckets (16-byte records)
  int bkt_mult = 2;         // bucket capacity in units of the average list length the caller made room for
  rrtx::PinnedBuf mailbox;       // host-mapped words the finish kernel reports to: [0] overflow records of a call
  rrtx::DevBuf ws_ev_a, ws_ev_cnt, ws_confirm_args;   // per-wave entry slices, their counts, confirm arguments
  rrtx::DevBuf ws_recs;     // HitRec
  rrtx::DevBuf ws_counts;   // int32 count[nq], cursor[nq]
  rrtx::DevBuf ws_bsum;     // int64 per-256-query sums of count (first level of the offsets scan)
  rrtx::DevBuf ws_scalars;  // device scalars of the range search: two records used alternately
  rrtx::DevBuf ws_scalars_nn;  // ... of the nearest search
  int scalars_flip = 0;
  rrtx::DevBuf ws_tmp;      // list entries that did not fit their bucket, in CSR position
  rrtx::DevBuf ws_owner;    // int32 owner query of every CSR entry (extend_candidates)
  rrtx::DevBuf ws_dub_rec;  // 128-byte records of the steered Dubins edges of one chunk (kernels_dubins.hip)
  rrtx::DevBuf ws_dub_ckpt; // running-sum checkpoints of those edges, 12 doubles each (RRTX_OPT_DUBINS_TIME_COLUMN = 1)
  rrtx::DevBuf ws_out_off, ws_out_idx, ws_out_dist, ws_out_u8a, ws_out_u8b, ws_out_i32, ws_out_f64;
  rrtx::DevBuf ws_partial;  // nearest partials
  rrtx::DevBuf ws_thr;      // per-query thresholds
  rrtx::DevBuf ws_mask;     // per-call obstacle mask (packed order)
  rrtx::DevBuf ws_i32a, ws_i32b;  // staged index arrays
  rrtx::DevBuf ws_sph_lists;      // per sample: spheres its candidate edges can touch (+ counts)
  rrtx::DevBuf ws_poly_lists;     // per sample: polygons its candidate edges can reach (+ counts), uint16
  rrtx::DevBuf ws_self;           // rrtx_extend_candidates_self[_dubins]: sample table, its fp32 shadow, row counts, max |q - origin|

  // device mirror of the planner's directed edges (obstacle sweeps, kernels_sweep.hip)
  rrtx::DevArray<int32_t> ge_start, ge_end;
  rrtx::DevArray<double> ge_dist;   // edge.dist of every mirrored edge (Inf = blocked); SimpleEdge cost by default
  rrtx::DevArray<double> ge_dist0;  // edge.distOriginal: what append / set_dist wrote last (block leaves it alone)
  rrtx::DevArray<uint8_t> ge_dirty; // edge cost touched since the last cost solve (set_dist / block / cull)
  rrtx::GraphCost gc;               // cost propagation state (kernels_graph.hip)
  int64_t ge_n = 0, ge_cap = 0;
  rrtx::DevBuf ws_sweep_mark, ws_sweep_flag, ws_sweep_cnt, ws_sweep_start;
  // the batched sweep: obstacle table, in-range word per node, per-block lists of (edge id, hit word), counts per
  // (obstacle, block) and their scan, first CSR position of every group of 64 obstacles, the offsets
  rrtx::DevBuf ws_swb_tab, ws_swb_word, ws_swb_seg_id, ws_swb_seg_word, ws_swb_blk_n, ws_swb_cnt, ws_swb_pos, ws_swb_base, ws_swb_off;
  std::vector<rrtx::SweepObs> swb_tab_host;   // what ws_swb_tab is copied from (lives until the call's sync)
  // the batched release: one byte per packed active sphere, 1 = it stays (is not among the call's leaving obstacles)
  rrtx::DevBuf ws_rel_stay;
  std::vector<uint8_t> rel_stay_host;         // what ws_rel_stay is copied from (lives until the call's sync)
  // the batched polygon sweep: the groups' query tables (group g: pswb_qoff_host[g] .. [g + 1]), the packed table
  // position of every entry (-1: not in use), the candidates of a group (edge id, word of its start node, hit word)
  rrtx::DevBuf ws_pswb_q, ws_pswb_pos, ws_pswb_cand_id, ws_pswb_cand_word, ws_pswb_hit;
  std::vector<rrtx::SweepQueryOwned> pswb_q_host;   // what ws_pswb_q is copied from (lives until the call's sync)
  std::vector<int32_t> pswb_pos_host;               // what ws_pswb_pos is copied from (likewise)
  std::vector<int> pswb_qoff_host;
  // the batched polygon release: the obstacles that stay, as ranges [pb, pe) of packed table positions (pairs)
  rrtx::DevBuf ws_prel_stay;
  std::vector<int32_t> prel_stay_host;              // what ws_prel_stay is copied from (lives until the call's sync)

  // parent / rewire selection over the extend lists (kernels_select.hip)
  rrtx::DevArray<double> node_lmc;  // rrtLMC per node as rrtx_node_cost_set left it (+Inf: never set)
  int64_t node_lmc_cap = 0, node_lmc_n = 0;   // slots allocated; slots initialised (follows n_nodes)
  rrtx::DevBuf ws_sel_cnt;          // int32 rewire entries per sample
  rrtx::DevBuf ws_sel_blk;          // rrtx_extend_select: everything that is per sample, one block (SelectBlock, rrtx_capi.hip)
  rrtx::DevBuf ws_sel_rwn, ws_sel_rwv, ws_sel_lmc;   // ... its rewire lists and a caller-given rrtLMC array
  int64_t sel_list_cap = 0;         // ... entries its neighbour lists have room for
  // the lists the last successful rrtx_extend_select[_dubins] left in ws_out_idx / _dist / _u8a / _u8b and ws_sel_blk, for
  // rrtx_graph_edges_append_selected: its nq (-1: no such lists; every entry point that writes those workspaces drops
  // the record, CHECK_CTX in rrtx_capi.hip) and its entry count
  int sel_hold_nq = -1;
  int64_t sel_hold_count = 0;
  int sel_hold_cols = 1;            // ... 1: the one SimpleEdge cost column; 3: key | cost_out | cost_in (rrtx_extend_select_dubins)

  // neighbour lists -> mirror edges (kernels_link.hip): edges per row, their scan, {entries, edges, verdict}, the
  // staged node_of, and what rrtx_graph_edges_get gathers into
  rrtx::DevBuf ws_link_cnt, ws_link_row, ws_link_res, ws_link_node, ws_link_get;
  rrtx::DevBuf ws_delta_node;       // rrtx_graph_cost_update_delta: the changed nodes

  // move-target selection (kernels_target.hip): the two query blocks the rounds alternate between, each
  // [pose | radius | thr_lt, thr_gt | slot] of the poses still searching, and [results | pending | header]
  // (TargetQueryBlock and TargetResultBlock in rrtx_capi.hip describe them)
  rrtx::DevBuf ws_tgt_blk[2], ws_tgt_res;

  // radius -> threshold cache
  double thr_cache_r = -1.0, thr_cache_lt = 0.0, thr_cache_gt = 0.0;

  // profiling
  int profiling = 0;                // 0 off, 1 range-scan family only, 2 every family
  bool span_open = false;
  std::vector<rrtx::TimedSpan> spans;
  std::vector<hipEvent_t> event_pool;
  double fam_ms[rrtx::KF_COUNT] = {0};
  int64_t fam_launches[rrtx::KF_COUNT] = {0};
  int64_t last_pairs = 0, last_neighbors = 0;
  int last_tile_q = 0;
  bool last_culled = false;         // the last range search used the slab-culled scan
  int last_placement = 0;           // RRTX_OPT_LAST_PLACEMENT of the last range search
  int last_tile_form = 0;           // rrtx_last_tile_form: 0 none, 1 looped, 2 straight
  int64_t last_sweep_candidates = 0;
  int last_visit_slices = 0;        // entries of ws_ev_cnt holding its per-wave chunk counts

  // cull and compaction of the edge mirror (kernels_cull.hip).  Last in the context, so that no member above moves:
  // a byte per mirrored edge beside ge_dirty (1: rrtx_graph_edges_cull dropped the edge; zero at and beyond ge_n), and
  // the workspaces: a byte per node (1 = listed) and the staged list, counts per workgroup and their scan,
  // remap[old id], {a culled parent edge, the new solved_edges}
  rrtx::DevArray<uint8_t> ge_culled;
  rrtx::DevBuf ws_cull_map, ws_cull_nodes, ws_cull_cnt, ws_cull_pos, ws_cull_remap, ws_cull_res;

  ~rrtx_ctx();                      // what is not memory (rrtx_capi.hip); the members then release what they own
};

namespace rrtx {

int fail(rrtx_ctx *ctx, int code, const char *fmt, ...);

// roctx range for the duration of one C-ABI call (rrtx_capi.hip); a no-op without a marker library
struct ApiRange {
  explicit ApiRange(const char *name);
  ~ApiRange();
  bool active;
};

#define RRTX_HIP(ctx, expr)                                                               \
  do {                                                                                    \
    hipError_t _e = (expr);                                                               \
    if (_e != hipSuccess)                                                                 \
      return ::rrtx::fail((ctx), RRTX_E_DEVICE, "%s failed: %s (%s:%d)", #expr,           \
                          hipGetErrorString(_e), __FILE__, __LINE__);                     \
  } while (0)

// RRTX_OPT_TUNE decoded, in the one place that shifts and masks it (experiment switches: never change a result)
struct TuneBits {
  bool xy_order;       // bit 0: order the query copies by (x, y) bucket only (g3 = 1)
  bool whole_chunks;   // bit 1: the tile kernel lists whole chunks, never groups of eight positions
  bool place_pass;     // bit 2 (value 4): the place pass orders the copies even without ghosts
  bool loop_form;      // bit 3 (value 8): the tile kernel keeps its looped form where the straight one would run
  int kz_bins;         // bits 8-15: bins of the third coordinate inside a slab cell (0: kSlabKz)
  int g3_side;         // bits 16-20: side of the cubic grid of query buckets (0: from the batch size)
  int cell_shift;      // bits 24-25: slab cells of kSlabChunk >> cell_shift nodes
};
inline TuneBits tune_bits(const rrtx_ctx *ctx) {
  const int t = ctx->opt_tune;
  return TuneBits{(t & 1) != 0, (t & 2) != 0, (t & 4) != 0, (t & 8) != 0, (t >> 8) & 0xff, (t >> 16) & 0x1f, (t >> 24) & 3};
}

// One launch site per kernel template: fn (a generic lambda) gets the dimension as std::integral_constant<int, 3>
// or <int, 4>; combinations that are never launched are kept out with `if constexpr` at the call site.
template <class Fn>
inline void for_dim(int dim, Fn &&fn) {
  if (dim == 4) fn(std::integral_constant<int, 4>{});
  else fn(std::integral_constant<int, 3>{});
}

// profiling spans around a kernel family
void span_begin(rrtx_ctx *ctx, int family);
void span_end(rrtx_ctx *ctx);

// thresholds on squared distances (host, exact):
//   first_ge(r): smallest s >= 0 with sqrt(s) >= r   (sqrt(s) <  r  <=>  s <  first_ge(r))
//   first_gt(r): smallest s >= 0 with sqrt(s) >  r   (sqrt(s) <= r  <=>  s <  first_gt(r))
double thr_first_ge(double r);
double thr_first_gt(double r);
double thr_point_clear(double robot_radius, double radius);

// ---- a call's neighbour lists on the device, as ONE value ------------------------
// W: the columns may be written (Lists); read-only otherwise (ListsRO, what the selection and the link kernels get).
// The per-entry results of both directed edges of a list; null: the call has no such column.
template <bool W>
struct EdgeColsT {
  template <class T> using P = std::conditional_t<W, T, const T> *;
  P<double> cost_out, cost_in; P<uint8_t> word_out, word_in, hit_out, hit_in;
};
// The lists: the CSR (offsets of nq + 1 rows, *count = the entries the search produced, which may exceed cap), per entry
// the near index, the owner row, the key and the edge columns, and the entries every column has room for.  SimpleEdge has
// one double column, which is key, e.cost_out and e.cost_in alike.  A launcher reads the columns it needs and no other.
// INVARIANT: a view is built after the last ensure of every buffer it points into, and a function that receives a view
// ensures none of those buffers (ws_out_*, ws_owner, the block that holds offsets and count).  The SimpleEdge preamble
// (rrtx_extend_candidates[_dev]), the range search and the two SimpleEdge edge launchers take positional pointers.
template <bool W>
struct ListsT {
  template <class T> using P = std::conditional_t<W, T, const T> *;
  P<int64_t> offsets, count; P<int32_t> idx, owner; P<double> key; EdgeColsT<W> e; int64_t cap;
};
using EdgeCols = EdgeColsT<true>;
using Lists = ListsT<true>;
using ListsRO = ListsT<false>;
inline ListsRO read_only(const Lists &L) {
  return ListsRO{L.offsets, L.count, L.idx, L.owner, L.key,
                 {L.e.cost_out, L.e.cost_in, L.e.word_out, L.e.word_in, L.e.hit_out, L.e.hit_in}, L.cap};
}
// What idx points into: `rows` rows of a table the edge kernels read in their own layout (launch_candidate_edges and
// _polygons: four doubles a row; launch_candidate_dubins: four columns of `rows` doubles).  Null: the context's nodes.
struct NearTable { const double *p = nullptr; int64_t rows = 0; };
// The tree column of the closest calls: one entry a row, (row j, node tree_idx[j]).  tree_idx null: no such column.
struct TreeColumn { const int32_t *tree_idx; EdgeCols e; };

// ---- launchers (device pointers, enqueue on ctx->stream) ----------------------
// Fused extend() work of the range search (sphere list, culled search only): both directed edges of
// every list entry and explicitPointCheck of the samples; r = radius the lists are built with.
// `fused` tells the caller whether the search did it (otherwise: launch_candidate_edges).
struct ExtendFuse { double r; uint8_t *hit_out, *hit_in, *sample_unsafe; bool fused; };
// the last launch of the range search (kernels_finish.hip); device types passed as void *
struct FinishLaunch {
  const int *count; int nq; int bcap;
  const void *bkt; void *tmp; const void *ovf; long long ovf_cap; const void *scalars;
  bool prescattered;
  int64_t *offsets; int64_t *needed; int32_t *idx; double *dist; long long out_cap;
  int32_t *owner; int32_t *nearest_idx; double *nearest_dist;
  int *qhist; int n_qhist; unsigned *mailbox;
  const double *q; double r_start;
  uint8_t *hit_out, *hit_in;   // fused extend(): the records' edge flags go here (null: not fused)
};
int launch_nn_finish(rrtx_ctx *ctx, const FinishLaunch &f);
int launch_nn_radius(rrtx_ctx *ctx, const double *q_dev, const double *r_dev_or_null, double r_scalar,
                     int nq, int64_t *offsets_dev, int32_t *idx_dev, double *dist_dev, int64_t cap,
                     int64_t *needed_dev, int32_t *owner_dev = nullptr, int32_t *nearest_idx_dev = nullptr,
                     double *nearest_dist_dev = nullptr, ExtendFuse *ext = nullptr);
int knearest_row(int k, int64_t n_nodes);
int launch_nn_knearest(rrtx_ctx *ctx, const double *q_dev, int nq, int k, int32_t *idx_dev, double *dist_dev,
                       int32_t *count_dev);
int launch_nn_nearest(rrtx_ctx *ctx, const double *q_dev, int nq, int32_t *idx_dev, double *dist_dev,
                      bool exact = false);
int scan_units(rrtx_ctx *ctx, int *units);   // (tile, chunk) units of the last culled range scan
int slab_refresh(rrtx_ctx *ctx, long long n_tiles);
bool slab_run_wanted(const rrtx_ctx *ctx, int64_t n);
// what the append kernel needs to draw the (cell, rank) of every node of a sorted run (kernels_slab.hip)
// the grid of the slab index, written on the device at every rebuild (slab_params_kernel)
struct SlabParams { double x0, inv_wx, y0, inv_wy, z0, inv_wz; int Kx, Ky, Kz, pad; };
struct RunRank { const SlabParams *sp; int *hist; int2 *sr; };
int slab_run_prepare(rrtx_ctx *ctx, int64_t n, RunRank *rr);
int slab_append_run(rrtx_ctx *ctx, int64_t base, int64_t n);   // bring the slab index up to date when it pays (kernels_slab.hip)
constexpr int kSlabChunk = 512;              // node positions per chunk of the slab index
int launch_edges_spheres(rrtx_ctx *ctx, const double *p0_dev, const double *p1_dev, int64_t ne,
                         double robot_radius, int obstacle_or_minus1, int obs_begin, int obs_end,
                         uint8_t *hit_dev, int32_t *first_hit_dev, const int32_t *sidx_dev = nullptr,
                         const int32_t *eidx_dev = nullptr, const uint8_t *mask_host = nullptr);
int launch_edges_polygons(rrtx_ctx *ctx, const double *p0_dev, const double *p1_dev, int64_t ne,
                          double robot_radius, int obstacle_or_minus1, int obs_begin, int obs_end,
                          uint8_t *hit_dev, int32_t *first_hit_dev);
int launch_points_spheres(rrtx_ctx *ctx, const double *p_dev, int64_t np, double robot_radius, int quick,
                          uint8_t *unsafe_dev, double *clearance_dev);
int launch_points_polygons(rrtx_ctx *ctx, const double *p_dev, int64_t np, double robot_radius,
                           uint8_t *unsafe_dev, double *clearance_dev, double list_r = -1.0,
                           const unsigned short **lists_out = nullptr, const unsigned short **list_cnt_out = nullptr);
int launch_simple_steer(rrtx_ctx *ctx, const double *s_dev, const double *g_dev, int64_t ne,
                        double *dist_dev, double *wdist_dev);
int launch_dubins_steer(rrtx_ctx *ctx, const double *s_dev, const double *g_dev, int64_t ne, double r_min,
                        double *cost_dev, uint8_t *word_dev, double *wdist_dev = nullptr,
                        double *velocity_dev = nullptr, uint8_t *valid_dev = nullptr);
int launch_dubins_edges_check(rrtx_ctx *ctx, const double *s_dev, const double *g_dev, int64_t ne,
                              double r_min, double robot_radius, double *cost_dev, uint8_t *word_dev,
                              uint8_t *hit_dev, int32_t *traj_len_dev, int pb = -1, int pe = -1);
int launch_dubins_edges_idx(rrtx_ctx *ctx, const int32_t *ids_dev, int64_t n, double r_min, double robot_radius, int pb,
                            int pe, uint8_t *hit_dev);
int launch_sweep_mark_multi(rrtx_ctx *ctx, const SweepQuery *queries_host, int nqs);
int launch_sweep_select(rrtx_ctx *ctx, int blocked_only, int32_t *out_dev, long long cap, long long **total_dev);
int launch_sweep_finish(rrtx_ctx *ctx, const int32_t *ids_dev, long long n, const uint8_t *hit, const uint8_t *o1,
                        const uint8_t *o2, int32_t *out_dev, long long cap, long long **total_dev);
int launch_sweep_gather(rrtx_ctx *ctx, const int32_t *ids_dev, long long n, double *p0_dev, double *p1_dev);
void packed_range(const std::vector<int32_t> &orig, int begin, int end, int &pb, int &pe);
std::vector<int32_t> active_positions(const std::vector<uint8_t> &active);
// Candidate Dubins edges of extend(): both directed edges of every entry of L steered and checked into L.e (words may be
// null).  No sample pass; returns at cap <= 0.
int launch_candidate_dubins(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, double r_min, double robot_radius,
                            NearTable near = {});
int launch_detmath_eval(rrtx_ctx *ctx, int op, const double *x_dev, const double *y_dev, int64_t n, double *out_dev);
int launch_dubins_trajectory(rrtx_ctx *ctx, const double *s_dev, const double *g_dev, int64_t ne, double r_min,
                             const int64_t *traj_off_dev, double *traj_xy_dev, int64_t cap_rows,
                             int32_t *traj_len_dev);
// candidate edges of extend(): for every CSR entry both directed edges vs the sphere list.  idx[e] is a row of
// near_aos (four doubles a row, n_near rows): the context's nodes unless a table is given (the samples themselves,
// rrtx_extend_candidates_self)
int launch_candidate_edges(rrtx_ctx *ctx, const double *q_dev, int nq, const int64_t *offsets_dev,
                           const int32_t *idx_dev, const int32_t *owner_dev, int64_t cap, double robot_radius,
                           uint8_t *hit_out_dev, uint8_t *hit_in_dev, double r = -1.0,
                           uint8_t *sample_unsafe_dev = nullptr, const double *near_aos = nullptr, int64_t n_near = 0);
int launch_candidate_edges_polygons(rrtx_ctx *ctx, const double *q_dev, int nq, const int64_t *offsets_dev,
                                    const int32_t *idx_dev, const int32_t *owner_dev, int64_t cap,
                                    double robot_radius, uint8_t *hit_out_dev, uint8_t *hit_in_dev,
                                    uint8_t *sample_unsafe_dev, double r = -1.0, const double *near_aos = nullptr,
                                    int64_t n_near = 0);
// both directed edges of every entry of a view, for the calls that are not the SimpleEdge preamble (the self and closest
// calls, find_new_target): a dim = 4 context checks Dubins edges, a dim = 3 context SimpleEdges against the polygon list
// (opt_extend_polygons) or the spheres, without a sample pass
int launch_list_edges(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, double robot_radius, double r_min, double r,
                      NearTable near = {});
// the samples of a batch among themselves (kernels_self.hip): into L the CSR of the earlier samples within r of every
// sample, keys and owners; *L.count = entries found, no entry at or beyond L.cap is written.  *table_out = the samples
// as the near table of launch_candidate_edges
int launch_self_join(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, double r, const uint8_t *skip_dev,
                     NearTable *table_out);
// the same in [x y t theta] with the context's wrapped dimensions: the copies of the later sample against the earlier
// sample as it is, the key of the first copy that reaches it; *table_out = the near table of launch_candidate_dubins
int launch_self_join_dubins(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, double r, const uint8_t *skip_dev,
                            NearTable *table_out);
// the k nearest earlier samples of every wanted live sample (kernels_self.hip): L holds nq x k slots (offsets and count
// are not used; owner: the row of every slot), both edge flags of every slot against the whole obstacle list, and the
// same flags for (sample, node tree_idx) when a tree column is given; bounded by nq, k and the node count on the device
int launch_closest_self(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, int k, double robot_radius,
                        const uint8_t *skip_dev, const uint8_t *want_dev, int32_t *count_dev, const TreeColumn &tree);
// the same in [x y t theta] with the context's wrapped dimensions: rows by the minimum over the later sample's copies,
// per slot the key, both Dubins costs, words (may be null) and flag bytes, and the same fields of the tree column
int launch_closest_self_dubins(rrtx_ctx *ctx, const Lists &L, const double *q_dev, int nq, int k, double robot_radius,
                               double r_min, const uint8_t *skip_dev, const uint8_t *want_dev, int32_t *count_dev,
                               const TreeColumn &tree);
int launch_nearest_from_lists(rrtx_ctx *ctx, const ListsRO &L, int nq, int32_t *nearest_idx_dev, double *nearest_dist_dev);

int launch_obstacle_sweep(rrtx_ctx *ctx, const double centre[3], double thr_lt, double thr_gt, const SphRec &ob,
                          int active, int32_t *out_dev, int64_t cap, long long **total_dev);

// device side of rrtx_obstacle_sweep_batch / rrtx_obstacle_release_batch over ctx->swb_tab_host (k obstacles).  Both
// modes leave a CSR in ws_swb_off (k + 1 offsets) / out_dev (at most cap ids) and *total_dev = the ids of all rows.
// Sweep: row j = obstacle j's sweep.  release (every obstacle of the table marked in use, ctx->rel_stay_host filled,
// sync_spheres has run for the call's robot radius): row j = the blocked edges obstacle j hits and no staying sphere does.
int launch_sphere_burst(rrtx_ctx *ctx, int k, bool release, int32_t *out_dev, int64_t cap, long long **total_dev);

// device side of rrtx_obstacle_sweep_polygon_batch / rrtx_obstacle_release_polygon_batch over ctx->pswb_q_host /
// pswb_qoff_host / pswb_pos_host (k entries, the mirror is not empty, sync_polygons has run): the same CSR in ws_swb_off
// / out_dev / *total_dev, row j = entry j's mode-0 sweep.  release (ctx->prel_stay_host filled): row j = the blocked edges
// entry j hits and no obstacle of the stay ranges does.  Synchronises once per group of 64 entries (the candidate
// count); ctx->last_sweep_candidates = their sum.
int launch_polygon_burst(rrtx_ctx *ctx, int k, double r_min, double robot_radius, bool release, int32_t *out_dev, int64_t cap,
                         long long **total_dev);
// explicitEdgeCheck(S, edge::DubinsEdge, ob) of the n mirrored edges cand_id[c] against the obstacles whose bit is set in
// cand_word[c] (bit b = packed table position ppos_dev[b], b < kg): bit b of hit_word[c] = edge c collides with it.
// stay_dev / n_stay (the release; null / 0 otherwise): n_stay ranges [pb, pe) of packed table positions; an edge that
// collides with an obstacle of one of them loses its hit word.  The caller has run sync_polygons and dubins_check_space.
int launch_dubins_check_words(rrtx_ctx *ctx, const int32_t *cand_id, const unsigned long long *cand_word, int64_t n,
                              double r_min, double robot_radius, const int32_t *ppos_dev, int kg,
                              unsigned long long *hit_word, const int32_t *stay_dev = nullptr, int n_stay = 0);
int dubins_check_space(rrtx_ctx *ctx);   // moving obstacles in use need RRTX_OPT_SPACE_HAS_TIME (RRTX_E_STATE)

int launch_graph_edge_dist(rrtx_ctx *ctx, long long first, long long n);
int launch_graph_touch(rrtx_ctx *ctx, long long first, long long n);
// edge.dist = Inf (restore = false) or edge.distOriginal (restore = true) for the edges ids[i], all in [0, ge_n)
int launch_graph_block(rrtx_ctx *ctx, bool restore, const int32_t *ids_host, long long n);      // synchronises
int launch_graph_block_dev(rrtx_ctx *ctx, bool restore, const int32_t *ids_dev, long long n);   // ids already on the device
// cullCurrentNeighbors over the mirror and the removal of what it culled (kernels_cull.hip); both synchronise.
// cull: nodes_host null = every node, else k validated node indices; the mirror is not empty.  compact: remap_host null
// or room for ge_n ids; RRTX_E_STATE with nothing changed when a kept solve has a culled parent edge.
int launch_edges_cull(rrtx_ctx *ctx, double ball, const int32_t *nodes_host, long long k, int64_t *n_culled);
int launch_edges_compact(rrtx_ctx *ctx, int32_t *remap_host, int64_t *n_removed);
int launch_graph_cost(rrtx_ctx *ctx, int root, bool update, double *lmc_dev, int32_t *parent_dev, int *passes_out);
void graph_cost_forget(rrtx_ctx *ctx);
int launch_graph_delta(rrtx_ctx *ctx, int root, bool store, int32_t *node_dev, double *lmc_dev, int32_t *par_dev, long long cap,
                       int64_t **total_dev, int *passes_out);
int launch_graph_delta_advance(rrtx_ctx *ctx, int root);
void graph_delta_forget(rrtx_ctx *ctx);

int launch_pack_hits(rrtx_ctx *ctx, const uint8_t *hit_out, const uint8_t *hit_in, const int64_t *n_valid_dev,
                     int64_t cap, uint64_t *words);

// findBestParent + rewire test over the lists of the extend preamble (kernels_select.hip); device pointers
struct SelectLaunch {
  int nq;
  ListsRO lists;
  const uint8_t *sample_unsafe; const double *lmc; int64_t n_lmc;
  int32_t *parent_idx; int64_t *parent_entry; double *lmc_new; uint8_t *status;
  int64_t *rw_offsets; int32_t *rw_node; double *rw_value; int64_t rw_cap; int64_t *rw_needed_dev;
};
int launch_select(rrtx_ctx *ctx, const SelectLaunch &L);

// neighbour lists -> mirror edges (kernels_link.hip); device pointers.  launch_link_count leaves {surviving entries,
// edges, verdict} in ctx->ws_link_res and the CSR of every sample's edges in row_first (nq + 1); the caller reads the
// three words, refuses or grows the mirror, and launch_link_fill writes edges [first, first + total).
enum : unsigned {
  kLinkOverflow = 1,      // *lists.count > lists.cap
  kLinkBadNode = 2,       // node_of[j] >= the node count
  kLinkBadIndex = 4,      // a surviving entry's near node / batch position out of range
  kLinkBadOffsets = 8,    // offsets out of order or beyond cap
  kLinkTooMany = 16,      // one row yields more than 2^31 - 1 edges
};
struct LinkLists {
  int nq;
  ListsRO lists;
  const int32_t *node_of; bool idx_is_batch;
  int64_t *row_first;
};
int launch_link_count(rrtx_ctx *ctx, const LinkLists &L);
int launch_link_fill(rrtx_ctx *ctx, const LinkLists &L, long long first, long long total);
int launch_link_gather(rrtx_ctx *ctx, const int32_t *ids_dev, long long n, int32_t *start_dev, int32_t *end_dev,
                       double *dist_dev, double *dist0_dev);

// findNewTarget, one round (kernels_target.hip): the first minimum of lmc[node] + cost over the unblocked entries of
// every pose still searching, then the poses without one move on to the next round's query block with twice the radius
// (or leave as NOT_FOUND beyond r_max).  Device pointers; also the argument record of the two kernels.
struct TargetRound {
  int n_act, nq, round, dim;        // poses of this round; poses of the call; 1-based round; doubles per pose
  double r_max;
  const int64_t *offsets;           // CSR of the round over its n_act poses
  const int32_t *idx; const double *cost; const uint8_t *hit_out;
  const int64_t *n_valid; long long cap;      // entries the search produced; entries the list arrays hold
  const double *lmc; long long n_lmc;
  const double *q, *rad; const int32_t *slot; // this round's block: pose, radius, index of the pose in the call
  int32_t *pending;                 // n_act: -1 resolved, else the length of the list that gave no target
  double *cost_to_goal, *edge_dist, *radius_used; int32_t *target_idx, *rounds; uint8_t *status;   // nq each
  double *q_next, *rad_next, *thr_next; int32_t *slot_next;   // next round's block (thr_gt follows n_next thr_lt)
  int64_t *hdr;                     // [1] poses of the next round (-1: this round overflowed), [2] entries they had
};
int launch_target_round(rrtx_ctx *ctx, const TargetRound &T);
int node_cost_ensure(rrtx_ctx *ctx);   // ctx->node_lmc covers every node (new slots +Inf)
// a.regrow(count, keep) on the context's stream; RRTX_E_NOMEM when the allocation fails
template <class T>
int regrow(rrtx_ctx *ctx, DevArray<T> &a, int64_t count, int64_t keep) {
  const hipError_t e = a.regrow((size_t)count, (size_t)keep, ctx->stream);
  if (e == hipErrorOutOfMemory) return fail(ctx, RRTX_E_NOMEM, "hipMalloc of %lld array elements failed", (long long)count);
  RRTX_HIP(ctx, e);
  return RRTX_OK;
}

// make sure the packed obstacle tables on the device match the host truth
int sync_spheres(rrtx_ctx *ctx, double robot_radius);
int sync_polygons(rrtx_ctx *ctx);
int sync_polygon_grid(rrtx_ctx *ctx, double pad_needed);

}  // namespace rrtx
