// contracts.cpp -- the contracts and scripts of the kernels the drivers reach (fake_hip.hpp).  Compiled for the host
// with the library's own headers, so the records a kernel takes by value (ConfirmArgs, PackFused, ...) are read with the
// layout the library was built with; the three records that live in a .hip source are mirrored below.
//
// Every contract cites the lines its ranges were read from.  A contract is a reading of the kernel, not the kernel.
#include "contracts.hpp"

#include <cstddef>
#include <cstring>
#include <string>

#include "../../rrtqx_3d_amd/csrc/collide_device.hpp"
#include "../../rrtqx_3d_amd/csrc/nn_device.hpp"
#include "fake_hip.hpp"

namespace hostsim {

Scene scene;

namespace {
using fakehip::Launch;
using namespace rrtx;

// ---- records declared in a .hip source, mirrored (the static_asserts there do not reach here: keep in step) ----------
struct PolyCsr {                  // kernels_collide.hip:426-435
  const double *q; const int64_t *offsets; const int32_t *idx; const int32_t *owner; const double4 *nodes_aos;
  uint8_t *hit_in; long long cap; int nq, n_nodes;
};
struct PolyGrid {                 // kernels_collide.hip:1186-1191
  double x0, y0, inv_wx, inv_wy; int g; const int32_t *start; const uint16_t *items;
};
struct RunRankArg { const void *sp; int *hist; void *sr; };   // rrtx_internal.hpp:512 (RunRank)
struct FinishArgs {               // kernels_finish.hip:31-56
  const int *count; int nq, bcap; const BktRec *bkt; BktRec *tmp; const HitRec *ovf; long long ovf_cap; const Scalars *sc;
  int prescattered; int want_nearest_fix; int64_t *offsets; int64_t *needed; int32_t *idx; double *dist; long long out_cap;
  int32_t *owner; int32_t *nearest_idx; double *nearest_dist; int *qhist; int n_qhist; unsigned *mailbox; const double *q;
  uint8_t *hit_out, *hit_in; double r_start; NearestIndex ni;
};
struct EdgeSrc {                  // kernels_dubins.hip:1085-1100
  int mode; int dir; const double *s, *g; const double *q; const int64_t *offsets; const int32_t *idx, *owner; int nq;
  const int32_t *ids; const int32_t *es, *ee; long long first; const double *nx, *ny, *nz, *nw; int n_nodes; long long cap;
};
struct PolyTab {                  // kernels_dubins.hip:443-452
  const double *meta; const int32_t *off; const double *vxy; const double *vslope; const int32_t *poff; const double *path;
  const double *pbox; int m;
};
constexpr int kRecDoubles = 16;   // kernels_dubins.hip:1134
constexpr int kPolyListCap = 64;  // kernels_collide.hip:402
constexpr size_t kScalarsUsed = offsetof(Scalars, pad);   // the fields a kernel writes (nn_device.hpp:20-27; pad: never)

// the samples of the search under way: every search begins with the pack kernel, whose contract notes its nq
// (and its copies: nq times the copies a query has under the wrapped dimensions; the ghosts that are skipped are counted in)
int g_pack_nq = 0;
size_t g_pack_copies = 0;
int scene_nq() { return g_pack_nq; }

// SCRIPT of the flag bytes a driver looks at (sample_unsafe, the two edge flags): "no collision", so that what comes back
// is not what the workspace happened to hold
void zero_at_execution(Launch &L, uint8_t *p, size_t n) {
  if (p && n) L.script([p, n] { std::memset(p, 0, n); });
}

int dim_of(const Launch &L) { return std::strstr(L.kernel, "<4") ? 4 : 3; }
size_t qrec(int D) { return D == 4 ? sizeof(QRec4) : sizeof(QRec3); }
size_t qrecf(int D) { return D == 4 ? sizeof(QRecF4) : sizeof(QRecF3); }

// the polygon tables a kernel walks over obstacles [0, m): sync_polygons packs them (kernels_collide.hip:1590-1608)
void polygon_tables(Launch &L, const double *meta, const int32_t *off, const double *vxy, int m) {
  if (m <= 0) return;               // (an empty list has no tables: null pointers, and no kernel loop looks at one)
  L.reads(meta, 32 * (size_t)m, "meta");
  L.reads(off, 4 * ((size_t)m + 1), "off");
  L.reads(vxy, 16 * (size_t)scene.poly_nv, "vxy");
}
void polygon_paths(Launch &L, const int32_t *path_off, const double *path, int m, int has_moving) {
  if (!has_moving) return;
  L.reads(path_off, 4 * ((size_t)m + 1), "path_off");
  L.reads(path, 24 * (size_t)scene.poly_rows, "path");
}

// rrtx_capi.hip:143-226.  i < n: pos[i * dim + k]; x / y / z / xf / ... [base + i]; the slab copies unless slab_later;
// aos as double4 [base + i]; chunk extents of the chunks of [base, base + n) by atomics; absmax, xrange[0..5] by atomics.
void aos_to_soa(Launch &L) {
  const int dim = L.arg<int>(1);
  const long long n = L.arg<long long>(2), base = L.arg<long long>(3);
  const int later = L.arg<int>(31);
  L.reads(L.ptr<double>(0), 8 * (size_t)dim * n, "pos");
  const int nd = dim == 4 ? 4 : 3;
  for (int k = 0; k < nd; ++k) {
    L.writes(L.ptr<double>(8 + k) + base, 8 * (size_t)n, "nodes[k]");
    L.writes(L.ptr<float>(12 + k) + base, 4 * (size_t)n, "nodes_f[k]");
    if (!later) {
      L.writes(L.ptr<float>(18 + k) + base, 4 * (size_t)n, "sl_f[k]");
      L.writes(L.ptr<double>(24 + k) + base, 8 * (size_t)n, "sl_d[k]");
    }
  }
  L.writes(L.ptr<float>(16) + base, 4 * (size_t)n, "nodes_pp");
  L.updates(L.ptr<char>(17), 8, "absmax");
  if (!later) {
    L.writes(L.ptr<float>(22) + base, 4 * (size_t)n, "sl_pp");
    L.writes(L.ptr<int32_t>(23) + base, 4 * (size_t)n, "sl_id");
    const long long c0 = base / kSlabChunk, c1 = (base + n - 1) / kSlabChunk;
    L.updates(L.ptr<char>(29) + 32 * c0, 32 * (size_t)(c1 - c0 + 1), "chunk_ext");
  } else {
    const RunRankArg rr = L.arg<RunRankArg>(32);
    L.reads(rr.sp, sizeof(SlabParams), "rr.sp");
    L.scratch(rr.sr, 8 * (size_t)n, "rr.sr");
  }
  L.writes(L.ptr<double>(28) + 4 * base, 32 * (size_t)n, "nodes_aos");
  L.updates(L.ptr<char>(30), 48, "xrange");
}

// kernels_graph.hip:58-68.  i < n: es / ee [first + i] -> rows of naos; dist, dist0, dirty [first + i].
void graph_edge_dist(Launch &L) {
  const long long first = L.arg<long long>(2), n = L.arg<long long>(3);
  L.reads(L.ptr<int32_t>(0) + first, 4 * (size_t)n, "ge_start");
  L.reads(L.ptr<int32_t>(1) + first, 4 * (size_t)n, "ge_end");
  L.reads(L.ptr<double>(5), 32 * (size_t)scene.n_nodes, "nodes_aos");
  L.writes(L.ptr<double>(6) + first, 8 * (size_t)n, "ge_dist");
  L.writes(L.ptr<double>(7) + first, 8 * (size_t)n, "ge_dist0");
  L.writes(L.ptr<uint8_t>(8) + first, (size_t)n, "ge_dirty");
}

// kernels_collide.hip:53-115.  i < ne: p0 / p1 [i * stride + 0..2], or sidx / eidx [i] -> nx / ny / nz; obstacles
// j in [m_begin, m_end): reach[j], sph[j], maskp[j], orig[j]; hit[i], first_hit[i] (null: not wanted).
void edges_spheres(Launch &L) {
  const int stride = L.arg<int>(2);
  const long long ne = L.arg<long long>(8);
  const int mb = L.arg<int>(13), me = L.arg<int>(14);
  if (L.ptr<int32_t>(3)) {
    L.reads(L.ptr<int32_t>(3), 4 * (size_t)ne, "sidx");
    L.reads(L.ptr<int32_t>(4), 4 * (size_t)ne, "eidx");
    for (int k = 0; k < 3; ++k) L.reads(L.ptr<double>(5 + k), 8 * (size_t)scene.n_nodes, "nodes[k]");
  } else {
    L.reads(L.ptr<double>(0), 8 * (size_t)stride * ne, "p0");
    L.reads(L.ptr<double>(1), 8 * (size_t)stride * ne, "p1");
  }
  const size_t m = (size_t)(me - mb);
  L.reads(L.ptr<SphRec>(9) + mb, 32 * m, "sph");
  L.reads(L.ptr<SphRec>(10) + mb, 32 * m, "reach");
  if (L.ptr<uint8_t>(11)) L.reads(L.ptr<uint8_t>(11) + mb, m, "maskp");
  L.reads(L.ptr<int32_t>(12) + mb, 4 * m, "orig");
  L.writes(L.ptr<uint8_t>(15), (size_t)ne, "hit");
  L.writes(L.ptr<int32_t>(16), 4 * (size_t)ne, "first_hit", true);
}

// kernels_collide.hip:238-275.  i < np: p[i * stride + 0..2]; j < m: sph[j], thr_in[j], radius[j]; unsafe[i],
// clearance[i] (null: not wanted).
void points_spheres(Launch &L) {
  const int stride = L.arg<int>(1), m = L.arg<int>(6);
  const long long np = L.arg<long long>(2);
  L.reads(L.ptr<double>(0), 8 * (size_t)stride * np, "p");
  L.reads(L.ptr<SphRec>(3), 32 * (size_t)m, "sph", m == 0);
  L.reads(L.ptr<double>(4), 8 * (size_t)m, "radius", m == 0);
  L.reads(L.ptr<double>(5), 8 * (size_t)m, "thr_in", m == 0);
  L.writes(L.ptr<uint8_t>(9), (size_t)np, "unsafe");
  L.writes(L.ptr<double>(10), 8 * (size_t)np, "clearance", true);
}

// kernels_collide.hip:1388-1398.  i < ne: s[i * dim + k], g[i * dim + k], k < dim (dim 3: k < 3); dist[i], wdist[i]
// (null: not wanted).
void simple_steer(Launch &L) {
  const int dim = L.arg<int>(2);
  const long long ne = L.arg<long long>(3);
  L.reads(L.ptr<double>(0), 8 * (size_t)dim * ne, "s");
  L.reads(L.ptr<double>(1), 8 * (size_t)dim * ne, "g");
  L.writes(L.ptr<double>(4), 8 * (size_t)ne, "dist", true);
  L.writes(L.ptr<double>(5), 8 * (size_t)ne, "wdist", true);
}

// kernels_collide.hip:291-337.  i < np: p[i * stride + 0..2]; tab[j], j < m; unsafe[i] (null: not wanted), list_n[i],
// lists[i * kSphListCap + c] for c < min(n, kSphListCap) only: the list array is the kernels' own scratch.
void sample_spheres(Launch &L) {
  const int stride = L.arg<int>(1), m = L.arg<int>(4);
  const long long np = L.arg<long long>(2);
  L.reads(L.ptr<double>(0), 8 * (size_t)stride * np, "p");
  L.reads(L.ptr<double>(3), 64 * (size_t)m, "tab");
  L.writes(L.ptr<uint8_t>(6), (size_t)np, "unsafe", true);
  zero_at_execution(L, L.ptr<uint8_t>(6), (size_t)np);
  L.scratch(L.ptr<int32_t>(7), 4 * (size_t)np * kSphListCap, "lists");
  L.writes(L.ptr<int32_t>(8), 4 * (size_t)np, "list_n");
}

// kernels_collide.hip:120-236.  offsets[nq] alone of the CSR; total > cap: returns.  e < total: owner[e], idx[e],
// q[owner * stride + 0..2], naos[idx]; list_n[owner], lists[owner * list_cap + c]; sph[j], j < m; reach_f in groups of
// eight obstacles (32 floats a group); hit_out[e], hit_in[e].
void candidate_edges(Launch &L) {
  const int stride = L.arg<int>(1), nq = L.arg<int>(3), n_nodes = L.arg<int>(7), m = L.arg<int>(14);
  const long long cap = L.arg<long long>(8);
  const long long total = scene.total;
  L.reads(L.ptr<int64_t>(2) + nq, 8, "offsets[nq]");
  if (total > cap) return;
  L.reads(L.ptr<double>(0), 8 * (size_t)stride * nq, "q");
  L.reads(L.ptr<int32_t>(4), 4 * (size_t)total, "idx");
  L.reads(L.ptr<int32_t>(5), 4 * (size_t)total, "owner");
  L.reads(L.ptr<double>(6), 32 * (size_t)n_nodes, "naos");
  L.reads(L.ptr<SphRec>(9), 32 * (size_t)m, "sph", m == 0);
  L.reads(L.ptr<float>(10), 4 * 32 * (size_t)((m + 7) / 8), "reach_f", m == 0);
  if (L.ptr<int32_t>(15)) {
    L.reads_unchecked(L.ptr<int32_t>(15), 4 * (size_t)nq * L.arg<int>(17), "lists");
    L.reads(L.ptr<int32_t>(16), 4 * (size_t)nq, "list_n");
  }
  L.writes(L.ptr<uint8_t>(19), (size_t)total, "hit_out");
  L.writes(L.ptr<uint8_t>(20), (size_t)total, "hit_in");
  zero_at_execution(L, L.ptr<uint8_t>(19), (size_t)total);
  zero_at_execution(L, L.ptr<uint8_t>(20), (size_t)total);
}

// kernels_collide.hip:935-957 and its wave function 458-927.  Unpaired: i < ne: p0 / p1 [i * stride + 0..1] (+ 2 with
// obstacles that move); obstacles j < m_end: meta[4 j ..], off[j], off[j + 1], vxy / vslope by vertex, path_off / path
// when they move, orig[j]; hit[i], first_hit[i] (null: not wanted).  Paired (the CSR of extend): csr.offsets[nq];
// owner[i], idx[i] for every i < cap BEFORE the list length is known (:479-480, :496-498), used for i < total only;
// q, nodes_aos; near_cnt / near_lists of the sample pass; hit[i], csr.hit_in[i] for i < total.
void edges_polygons(Launch &L) {
  const bool paired = std::strstr(L.kernel, "edges_polygons_kernel<true") != nullptr;
  const int stride = L.arg<int>(2), has_moving = L.arg<int>(11), me = L.arg<int>(14);
  polygon_tables(L, L.ptr<double>(5), L.ptr<int32_t>(6), L.ptr<double>(7), me);
  L.reads(L.ptr<double>(8), 8 * (size_t)scene.poly_nv, "vslope");
  polygon_paths(L, L.ptr<int32_t>(9), L.ptr<double>(10), me, has_moving);
  L.reads(L.ptr<int32_t>(12), 4 * (size_t)me, "orig");
  if (!paired) {
    const long long ne = L.arg<long long>(3);
    L.reads(L.ptr<double>(0), 8 * (size_t)stride * ne, "p0");
    L.reads(L.ptr<double>(1), 8 * (size_t)stride * ne, "p1");
    L.writes(L.ptr<uint8_t>(16), (size_t)ne, "hit");
    L.writes(L.ptr<int32_t>(17), 4 * (size_t)ne, "first_hit", true);
    return;
  }
  const PolyCsr c = L.arg<PolyCsr>(4);
  const long long total = scene.total;
  L.reads(c.offsets + c.nq, 8, "csr.offsets[nq]");
  L.reads_unchecked(c.owner, 4 * (size_t)c.cap, "csr.owner");
  L.reads_unchecked(c.idx, 4 * (size_t)c.cap, "csr.idx");
  if (total > c.cap) return;
  L.reads(c.owner, 4 * (size_t)total, "csr.owner (entries)");
  L.reads(c.idx, 4 * (size_t)total, "csr.idx (entries)");
  L.reads(c.q, 8 * (size_t)stride * c.nq, "csr.q");
  L.reads(c.nodes_aos, 32 * (size_t)c.n_nodes, "csr.nodes_aos");
  if (L.ptr<uint16_t>(18)) {
    L.reads_unchecked(L.ptr<uint16_t>(18), 2 * (size_t)c.nq * kPolyListCap, "near_lists");
    L.reads(L.ptr<uint16_t>(19), 2 * (size_t)c.nq, "near_cnt");
  }
  L.writes(L.ptr<uint8_t>(16), (size_t)total, "hit");
  L.writes(c.hit_in, (size_t)total, "csr.hit_in");
  zero_at_execution(L, L.ptr<uint8_t>(16), (size_t)total);
  zero_at_execution(L, c.hit_in, (size_t)total);
}

// kernels_collide.hip:1171-1183 and point_full_loop 1060-1169.  i < np: p[i * stride + 0..1] (+ 2 with obstacles that
// move); obstacles j < m as above; unsafe[i], clearance[i] (null: not wanted).
void points_polygons(Launch &L) {
  const int stride = L.arg<int>(1), has_moving = L.arg<int>(8), m = L.arg<int>(9);
  const long long np = L.arg<long long>(2);
  L.reads(L.ptr<double>(0), 8 * (size_t)stride * np, "p");
  polygon_tables(L, L.ptr<double>(3), L.ptr<int32_t>(4), L.ptr<double>(5), m);
  polygon_paths(L, L.ptr<int32_t>(6), L.ptr<double>(7), m, has_moving);
  L.writes(L.ptr<uint8_t>(11), (size_t)np, "unsafe", true);
  zero_at_execution(L, L.ptr<uint8_t>(11), (size_t)np);
  L.writes(L.ptr<double>(12), 8 * (size_t)np, "clearance", true);
}

// kernels_collide.hip:1209-1386.  i < np: p[i * stride + 0..1]; obstacles j < m: meta, off, vxy, bbox[4 j ..]; ytab[k],
// k < n_ytab; the grid's cell starts (g * g + 1) and the items they delimit; unsafe[i] (null: the lists alone);
// list_cnt[i] and the first entries of lists[i * kPolyListCap ..]: the list array is the kernels' own scratch.
void points_polygons_flag(Launch &L) {
  const int stride = L.arg<int>(1), m = L.arg<int>(6), n_ytab = L.arg<int>(11);
  const long long np = L.arg<long long>(2);
  L.reads(L.ptr<double>(0), 8 * (size_t)stride * np, "p");
  polygon_tables(L, L.ptr<double>(3), L.ptr<int32_t>(4), L.ptr<double>(5), m);
  L.writes(L.ptr<uint8_t>(8), (size_t)np, "unsafe", true);
  zero_at_execution(L, L.ptr<uint8_t>(8), (size_t)np);
  L.reads(L.ptr<double>(9), 32 * (size_t)m, "bbox");
  L.reads(L.ptr<double>(10), 8 * (size_t)(n_ytab > 0 ? n_ytab : 0), "ytab", n_ytab <= 0);
  if (L.ptr<uint16_t>(13)) {
    L.scratch(L.ptr<uint16_t>(13), 2 * (size_t)np * kPolyListCap, "lists");
    L.writes(L.ptr<uint16_t>(14), 2 * (size_t)np, "list_cnt");
  }
  const PolyGrid g = L.arg<PolyGrid>(15);
  if (g.g > 0) {
    const size_t cells = (size_t)g.g * g.g;
    L.reads(g.start, 4 * (cells + 1), "grid.start");
    // (uploaded by a synchronous copy before this launch, sync_polygon_grid: the last start is there to be read)
    L.reads(g.items, 2 * (size_t)g.start[cells], "grid.items");
  }
}

// ---- the range search without culling (small trees): pack, prep, scan, confirm, finish -------------------------------

// nn_device.hpp:259-403.  i < nq: q[i * D + k]; thr arrays [i] (null: the scalars); with pf.count: count[i], count[nq],
// *ca_dst, the next call's Scalars record, node 0 of pf.nx.., and entry 0 of the sample's bucket when the root rule adds
// it; slots only with ghosts; copies[pos], meta[pos], pos < nq; sc: n_copies stored, q_absmax by atomic.
void nn_pack(Launch &L) {
  const int D = dim_of(L), nq = L.arg<int>(1), n_wraps = L.arg<int>(6);
  const size_t n_slots = (size_t)1 << n_wraps;
  g_pack_nq = nq;
  g_pack_copies = (size_t)nq * n_slots;
  L.reads(L.ptr<double>(0), 8 * (size_t)D * nq, "q");
  L.reads(L.ptr<double>(2), 8 * (size_t)nq, "thr_lt", true);
  L.reads(L.ptr<double>(3), 8 * (size_t)nq, "thr_gt", true);
  const PackFused pf = L.arg<PackFused>(26);
  const ConfirmArgs ca = L.arg<ConfirmArgs>(27);
  const QSlots qs = L.arg<QSlots>(28);
  const PackSamples ps = L.arg<PackSamples>(29);
  if (qs.tab || ps.out || L.ptr<int>(24))
    fakehip::finding("NOCONTRACT %s on the culled route (bucket-slot table, sample role): not driven", L.kernel);
  if (pf.count) {
    L.writes(pf.count, 4 * ((size_t)nq + 1), "pf.count");
    L.writes(pf.ca_dst, sizeof(ConfirmArgs), "pf.ca_dst");
    L.writes(pf.sc_next, kScalarsUsed, "pf.sc_next");
    L.reads(pf.nx, 8, "pf.nx[0]"); L.reads(pf.ny, 8, "pf.ny[0]"); L.reads(pf.nz, 8, "pf.nz[0]");
    if (D == 4) L.reads(pf.nw, 8, "pf.nw[0]");
    L.scratch(ca.hs.bkt, 16 * (size_t)nq * ca.hs.bcap, "ca.hs.bkt");
  }
  if (n_wraps > 0) L.writes(L.ptr<char>(17), sizeof(SlotRec) * nq * n_slots, "slots");
  L.writes(L.ptr<char>(18), qrec(D) * nq * n_slots, "copies");
  L.writes(L.ptr<char>(19), 8 * (size_t)nq * n_slots, "meta");
  L.updates(L.ptr<char>(20), kScalarsUsed, "sc");
}

// nn_device.hpp:509-524.  i < n_copies: copies[i] -> copies_f[i]; then records that never pass up to the next multiple
// of kQPI; sc->n_copies, sc->q_absmax, *node_absmax.
void nn_filter_prep(Launch &L) {
  const int D = dim_of(L), n = L.arg<int>(3);
  L.reads(L.ptr<char>(0), qrec(D) * (size_t)n, "copies");
  L.reads(L.ptr<char>(1), kScalarsUsed, "sc");
  L.reads(L.ptr<char>(2), 8, "node_absmax");
  L.writes(L.ptr<char>(8), qrecf(D) * (size_t)((n + kQPI - 1) / kQPI * kQPI), "copies_f");
}

// kernels_nn.hip:428-460 (scan_chunk_f32: 303-391).  fx / fy / fz / fw / fpp [id], id < n_nodes (clamped); copies_f
// kQPI records at a time up to the padded count; the wave's slice ev[slice * slice_cap ..] (scratch), ev_cnt[slice],
// slice < 4 * gridDim.x; *ca when a slice is drained (its sinks are those of nn_confirm_kernel).
void nn_scan_f32(Launch &L) {
  const int D = dim_of(L), n_nodes = L.arg<int>(5), slice_cap = L.arg<int>(13);
  const size_t n_slices = (size_t)L.grid.x * (kScanThreads / 64);
  for (int k = 0; k < (D == 4 ? 4 : 3); ++k) L.reads(L.ptr<float>(k), 4 * (size_t)n_nodes, "nodes_f[k]");
  L.reads(L.ptr<float>(4), 4 * (size_t)n_nodes, "nodes_pp");
  L.reads(L.ptr<char>(6), qrecf(D) * ((g_pack_copies + kQPI - 1) / kQPI * kQPI), "copies_f");
  L.reads(L.ptr<char>(10), kScalarsUsed, "sc");
  L.scratch(L.ptr<char>(11), 8 * n_slices * slice_cap, "ev");
  L.writes(L.ptr<int>(12), 4 * n_slices, "ev_cnt");
  L.reads(L.ptr<char>(14), sizeof(ConfirmArgs), "ca");
}

// kernels_nn.hip:262-282 (confirm_entry: 160-260).  ev_cnt[w], ev[w * slice_cap + e], w < n_slices; the nodes by
// position, the copies and their owners; hits: count[owner] by atomic, the owner's bucket, the overflow list and
// sc->total.
void nn_confirm(Launch &L) {
  const int D = dim_of(L), n_slices = L.arg<int>(3), slice_cap = L.arg<int>(4), n_nodes = L.arg<int>(5);
  const ConfirmArgs a = L.arg<ConfirmArgs>(0);
  const size_t nq = (size_t)scene_nq();
  L.reads(L.ptr<int>(2), 4 * (size_t)n_slices, "ev_cnt");
  L.reads_unchecked(L.ptr<char>(1), 8 * (size_t)n_slices * slice_cap, "ev");
  L.reads(a.nx, 8 * (size_t)n_nodes, "a.nx"); L.reads(a.ny, 8 * (size_t)n_nodes, "a.ny");
  L.reads(a.nz, 8 * (size_t)n_nodes, "a.nz");
  if (D == 4) L.reads(a.nw, 8 * (size_t)n_nodes, "a.nw");
  L.reads(a.copies, qrec(D) * nq * a.n_slots, "a.copies");
  L.reads(a.meta, 8 * nq * a.n_slots, "a.meta");
  if (a.n_slots > 1) L.reads(a.slots, sizeof(SlotRec) * nq * a.n_slots, "a.slots");
  L.updates(a.hs.count, 4 * nq, "a.hs.count");
  L.scratch(a.hs.bkt, 16 * nq * a.hs.bcap, "a.hs.bkt");
  L.scratch(a.hs.recs, 16 * (size_t)a.hs.cap, "a.hs.recs");
  L.updates(a.hs.sc, kScalarsUsed, "a.hs.sc");
}

// kernels_finish.hip:94-482.  count[q], the buckets, the overflow list, tmp (scratch, out_cap records); offsets[0..nq],
// *needed; idx / dist / owner [e] for e < min(total, out_cap) and no entry at or beyond out_cap; nearest_idx / _dist [q]
// (null: not wanted), for an empty ball through the slab index (ni) and q; qhist re-zeroed; mailbox[0] (host-mapped).
// SCRIPT: scene.total entries dealt over the samples, every one node (e mod n_nodes), owners in order.
void nn_finish(Launch &L) {
  const int D = dim_of(L);
  const FinishArgs a = L.arg<FinishArgs>(0);
  const size_t nq = (size_t)a.nq;
  const long long total = scene.total;
  const size_t n_out = (size_t)(total < a.out_cap ? total : a.out_cap);
  L.reads(a.count, 4 * nq, "count");
  L.reads_unchecked(a.bkt, 16 * nq * a.bcap, "bkt");
  L.reads_unchecked(a.ovf, 16 * (size_t)a.ovf_cap, "ovf");
  L.scratch(a.tmp, 16 * (size_t)(a.out_cap > 0 ? a.out_cap : 1), "tmp");
  L.reads(a.sc, kScalarsUsed, "sc");
  L.writes(a.offsets, 8 * (nq + 1), "offsets");
  L.writes(a.needed, 8, "needed");
  L.writes(a.idx, 4 * n_out, "idx", n_out == 0);
  L.writes(a.dist, 8 * n_out, "dist", n_out == 0);
  L.writes(a.owner, 4 * n_out, "owner", true);
  L.writes(a.nearest_idx, 4 * nq, "nearest_idx", true);
  L.writes(a.nearest_dist, 8 * nq, "nearest_dist", true);
  if (a.want_nearest_fix) {
    L.reads(a.q, 8 * (size_t)D * nq, "q");
    L.reads(a.ni.sx, 8 * (size_t)a.ni.n_nodes, "ni.sx"); L.reads(a.ni.sy, 8 * (size_t)a.ni.n_nodes, "ni.sy");
    L.reads(a.ni.sz, 8 * (size_t)a.ni.n_nodes, "ni.sz");
    L.reads(a.ni.sid, 4 * (size_t)a.ni.n_nodes, "ni.sid");
    L.reads(a.ni.chunk_ext, 32 * (size_t)a.ni.n_chunks, "ni.chunk_ext");
  }
  if (a.n_qhist > 0) L.writes(a.qhist, 4 * (size_t)a.n_qhist, "qhist");
  if (a.hit_out) { L.writes(a.hit_out, n_out, "hit_out"); L.writes(a.hit_in, n_out, "hit_in"); }
  L.writes_mapped(a.mailbox, 4, "mailbox[0]");
  const long long n_nodes = scene.n_nodes;
  const int miss = scene.nearest_miss_every;
  L.script([a, total, n_out, n_nodes, miss] {
    const long long nq = a.nq, each = total / nq, more = total % nq;
    long long at = 0;
    for (long long q = 0; q < nq; ++q) {
      a.offsets[q] = at;
      const long long len = each + (q < more ? 1 : 0);
      for (long long e = at; e < at + len && e < (long long)n_out; ++e) {
        a.idx[e] = (int32_t)(e % n_nodes);
        a.dist[e] = 1.0;
        if (a.owner) a.owner[e] = (int32_t)q;
      }
      at += len;
    }
    a.offsets[nq] = total;
    *a.needed = total;
    for (long long q = 0; q < nq; ++q) {
      if (a.nearest_idx) a.nearest_idx[q] = (miss > 0 && q % miss == 0) ? -1 : 0;
      if (a.nearest_dist) a.nearest_dist[q] = 1.0;
    }
    a.mailbox[0] = 0u;
  });
}

// ---- the nearest search (the host form's fallback for a nearest index of -1) ------------------------------------------

// nn_device.hpp:77-90.  *sc (every field but pad), the three fills, *ca_dst (null here).
void nn_init(Launch &L) {
  L.writes(L.ptr<char>(0), kScalarsUsed, "sc");
  L.writes(L.ptr<int>(2), 4 * (size_t)L.arg<int>(3), "zero_i32");
  L.writes(L.ptr<char>(4), 8 * (size_t)L.arg<int>(5), "fill_u64");
  L.writes(L.ptr<int>(7), 4 * (size_t)L.arg<int>(8), "fill_i32");
  L.writes(L.ptr<char>(10), sizeof(ConfirmArgs), "ca_dst", true);
}

// kernels_nearest.hip:151-251.  The node arrays in fp64 and fp32 over [0, n_nodes); copies / copies_f / meta [copy],
// copy < sc->n_copies; *node_absmax; candidates to recs (scratch, cap records) and sc->total; best_bits[owner] by atomic;
// redo[owner].
void nn_nearest_f32(Launch &L) {
  const int D = dim_of(L), n_nodes = L.arg<int>(9);
  const size_t nq = (size_t)scene_nq();
  for (int k = 0; k < (D == 4 ? 4 : 3); ++k) {
    L.reads(L.ptr<double>(k), 8 * (size_t)n_nodes, "nodes[k]");
    L.reads(L.ptr<float>(4 + k), 4 * (size_t)n_nodes, "nodes_f[k]");
  }
  L.reads(L.ptr<float>(8), 4 * (size_t)n_nodes, "nodes_pp");
  L.reads(L.ptr<char>(10), qrec(D) * g_pack_copies, "copies");
  L.reads(L.ptr<char>(11), qrecf(D) * g_pack_copies, "copies_f");
  L.reads(L.ptr<char>(12), 8 * g_pack_copies, "meta");
  L.reads(L.ptr<char>(13), 8, "node_absmax");
  L.scratch(L.ptr<char>(16), 16 * (size_t)L.arg<long long>(17), "recs");
  L.updates(L.ptr<char>(18), kScalarsUsed, "sc");
  L.updates(L.ptr<char>(19), 8 * nq, "best_bits");
  L.updates(L.ptr<int>(20), 4 * nq, "redo");
}
// kernels_nearest.hip:254-265.  recs[i], i < min(sc->total, cap); best_bits[owner]; best_idx[owner] by atomic.
void nn_nearest_tie(Launch &L) {
  const size_t nq = (size_t)scene_nq();
  L.reads_unchecked(L.ptr<char>(0), 16 * (size_t)L.arg<long long>(1), "recs");
  L.reads(L.ptr<char>(2), kScalarsUsed, "sc");
  L.reads(L.ptr<char>(3), 8 * nq, "best_bits");
  L.updates(L.ptr<int>(4), 4 * nq, "best_idx");
}
// kernels_nearest.hip:267-275.  i < nq: best_bits[i], best_idx[i] -> idx[i], dist[i].  SCRIPT: node 0 at distance 1.
void nn_nearest_out(Launch &L) {
  const int nq = L.arg<int>(2);
  L.reads(L.ptr<char>(0), 8 * (size_t)nq, "best_bits");
  L.reads(L.ptr<int>(1), 4 * (size_t)nq, "best_idx");
  int32_t *idx = L.ptr<int32_t>(3);
  double *dist = L.ptr<double>(4);
  L.writes(idx, 4 * (size_t)nq, "idx");
  L.writes(dist, 8 * (size_t)nq, "dist");
  L.script([idx, dist, nq] { for (int i = 0; i < nq; ++i) { idx[i] = 0; dist[i] = 1.0; } });
}
// kernels_nearest.hip:284-348.  sc->total; only beyond cap: redo[i], q[i * D + k], the slab index, idx[i], dist[i].
void nn_nearest_fixup(Launch &L) {
  const int D = dim_of(L), nq = L.arg<int>(4);
  const NearestIndex ni = L.arg<NearestIndex>(12);
  L.reads(L.ptr<char>(0), kScalarsUsed, "sc");
  L.reads(L.ptr<int>(2), 4 * (size_t)nq, "redo");
  L.reads(L.ptr<double>(3), 8 * (size_t)D * nq, "q");
  L.reads(ni.sx, 8 * (size_t)ni.n_nodes, "ni.sx"); L.reads(ni.sid, 4 * (size_t)ni.n_nodes, "ni.sid");
  L.reads(ni.chunk_ext, 32 * (size_t)ni.n_chunks, "ni.chunk_ext");
  L.updates(L.ptr<int32_t>(13), 4 * (size_t)nq, "idx");
  L.updates(L.ptr<double>(14), 8 * (size_t)nq, "dist");
}

// ---- the candidate Dubins edges of extend() (run_dubins_edges: a steering launch and two check launches a chunk) -------

// load_edge, mode 1 (kernels_dubins.hip:1110-1122): offsets[nq]; total > cap: nothing; entry i < total: owner[i], idx[i],
// the sample's row of q, the node's four coordinates.  Returns the entries of [base, base + count) that exist.
long long dubins_source(Launch &L, const EdgeSrc &s, long long base, long long count) {
  if (s.mode != 1) { fakehip::finding("NOCONTRACT %s with an edge source of mode %d: not driven", L.kernel, s.mode); return 0; }
  L.reads(s.offsets + s.nq, 8, "src.offsets[nq]");
  const long long total = scene.total;
  if (total > s.cap || total <= base) return 0;
  const long long n = (total - base < count) ? total - base : count;
  L.reads(s.owner + base, 4 * (size_t)n, "src.owner");
  L.reads(s.idx + base, 4 * (size_t)n, "src.idx");
  L.reads(s.q, 32 * (size_t)s.nq, "src.q");
  L.reads(s.nx, 8 * (size_t)s.n_nodes, "src.nx"); L.reads(s.ny, 8 * (size_t)s.n_nodes, "src.ny");
  L.reads(s.nz, 8 * (size_t)s.n_nodes, "src.nz"); L.reads(s.nw, 8 * (size_t)s.n_nodes, "src.nw");
  return n;
}
// kernels_dubins.hip:1175-1208.  k < count: the record of edge base + k at rec[16 k] (and rec2), stored by every lane of
// a wave that has an edge at all; cost[i], word[3 i ..] and their reverse twins for the edges i = base + k that exist.
void dubins_steer_rec(Launch &L) {
  const EdgeSrc s = L.arg<EdgeSrc>(0);
  const long long base = L.arg<long long>(1), count = L.arg<long long>(2);
  const long long n = dubins_source(L, s, base, count);
  if (n == 0) return;
  const size_t waves64 = (size_t)((n + 63) / 64 * 64 < count ? (n + 63) / 64 * 64 : count);
  L.scratch(L.ptr<double>(6), 8 * kRecDoubles * waves64, "rec");
  L.scratch(L.ptr<double>(10), 8 * kRecDoubles * waves64, "rec2", true);
  L.writes(L.ptr<double>(7) + base, 8 * (size_t)n, "cost", true);
  if (L.ptr<uint8_t>(8)) L.writes(L.ptr<uint8_t>(8) + 3 * base, 3 * (size_t)n, "word");
  if (L.ptr<int32_t>(9)) L.writes(L.ptr<int32_t>(9) + base, 4 * (size_t)n, "traj_len");
  if (L.ptr<double>(11)) L.writes(L.ptr<double>(11) + base, 8 * (size_t)n, "cost2");
  if (L.ptr<uint8_t>(12)) L.writes(L.ptr<uint8_t>(12) + 3 * base, 3 * (size_t)n, "word2");
}
// kernels_dubins.hip:1244-1271 (wave_dubins_collides: 600-1080).  The edges as above; rec[16 k] (rec[0] for a lane
// without an edge); the polygon list: meta, off, the vertices and their slopes, pbox, and the paths in a space with
// time; hit[base + k] for the edges that exist.  SCRIPT: no collision.
void dubins_check_rec(Launch &L) {
  const EdgeSrc s = L.arg<EdgeSrc>(0);
  const long long base = L.arg<long long>(1), count = L.arg<long long>(2);
  const PolyTab t = L.arg<PolyTab>(9);
  const long long n = dubins_source(L, s, base, count);
  if (n == 0) return;
  L.reads_unchecked(L.ptr<double>(10), 8 * kRecDoubles * (size_t)n, "rec");
  if (t.m > 0) {
    polygon_tables(L, t.meta, t.off, t.vxy, t.m);
    L.reads(t.vslope, 8 * (size_t)scene.poly_nv, "tab.vslope");
    L.reads(t.pbox, 32 * (size_t)t.m, "tab.pbox");
    polygon_paths(L, t.poff, t.path, t.m, scene.poly_rows > 0);
  }
  uint8_t *hit = L.ptr<uint8_t>(11) + base;
  L.writes(hit, (size_t)n, "hit");
  zero_at_execution(L, hit, (size_t)n);
}

}  // namespace

void register_contracts() {
  using fakehip::contract;
  contract("aos_to_soa_kernel", "rrtx_capi.hip:143-226", aos_to_soa);
  contract("graph_edge_dist_kernel", "kernels_graph.hip:58-68", graph_edge_dist);
  contract("edges_spheres_kernel", "kernels_collide.hip:53-115", edges_spheres);
  contract("points_spheres_kernel", "kernels_collide.hip:238-275", points_spheres);
  contract("simple_steer_kernel", "kernels_collide.hip:1388-1398", simple_steer);
  contract("sample_spheres_kernel", "kernels_collide.hip:291-337", sample_spheres);
  contract("candidate_edges_kernel", "kernels_collide.hip:120-236", candidate_edges);
  contract("edges_polygons_kernel", "kernels_collide.hip:458-957", edges_polygons);
  contract("points_polygons_flag_kernel", "kernels_collide.hip:1209-1386", points_polygons_flag);
  contract("points_polygons_kernel", "kernels_collide.hip:1060-1183", points_polygons);
  contract("nn_pack_kernel", "nn_device.hpp:259-403", nn_pack);
  contract("nn_filter_prep_kernel", "nn_device.hpp:509-524", nn_filter_prep);
  contract("nn_scan_f32_kernel", "kernels_nn.hip:303-391, 428-460", nn_scan_f32);
  contract("nn_confirm_kernel", "kernels_nn.hip:160-282", nn_confirm);
  contract("nn_finish_kernel", "kernels_finish.hip:94-482", nn_finish);
  contract("nn_init_kernel", "nn_device.hpp:77-90", nn_init);
  contract("nn_nearest_f32_kernel", "kernels_nearest.hip:151-251", nn_nearest_f32);
  contract("nn_nearest_tie_kernel", "kernels_nearest.hip:254-265", nn_nearest_tie);
  contract("nn_nearest_out_kernel", "kernels_nearest.hip:267-275", nn_nearest_out);
  contract("nn_nearest_fixup_kernel", "kernels_nearest.hip:284-348", nn_nearest_fixup);
  contract("dubins_steer_rec_kernel", "kernels_dubins.hip:1103-1130, 1175-1208", dubins_steer_rec);
  contract("dubins_check_rec_kernel", "kernels_dubins.hip:1103-1130, 1244-1271", dubins_check_rec);
}

}  // namespace hostsim
