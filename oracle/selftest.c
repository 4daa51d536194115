/* Address/UB-sanitised self test of the oracle (CPU only; GPU sanitizers are not available on the
 * pool).  Exercises every allocation path: kd-tree growth, range lists, ghost iterator, polygon and
 * Dubins code.  Build+run: make -C oracle selftest   (tests/test_oracle_sanitizer.py) */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "rrtx_oracle.h"

static double frand(unsigned *s) { *s = *s * 1664525u + 1013904223u; return (double)(*s >> 8) / 16777216.0; }

int main(void) {
  unsigned seed = 12345;
  int bad = 0;
  /* 3-D tree: kd == naive */
  orc_kd *t = orc_kd_create(3);
  for (int i = 0; i < 5000; ++i) { double p[3] = {frand(&seed), frand(&seed), frand(&seed)}; orc_kd_insert(t, p); }
  for (int k = 0; k < 200; ++k) {
    double q[3] = {frand(&seed), frand(&seed), frand(&seed)};
    int64_t a, b; double da, db;
    orc_kd_nearest(t, q, &a, &da); orc_kd_nearest_naive(t, q, &b, &db);
    bad += (a != b) || (da != db);
    orc_list *l = orc_kd_find_within_range(t, 0.15, q);
    orc_kd_find_more_within_range(t, 0.1, q, l);
    int32_t idx[4096]; double key[4096];
    int64_t n = orc_list_read(l, 4096, idx, key);
    int64_t m = orc_range_naive(t, 0.15, q, 0, NULL, NULL);
    bad += (n != m);
    orc_kd_empty_range_list(t, l);
  }
  orc_kd_destroy(t);
  /* wrapped 4-D tree */
  orc_kd *w = orc_kd_create(4);
  int wd[1] = {3}; double wp[1] = {2.0 * 3.141592653589793};
  orc_kd_set_wraps(w, 1, wd, wp);
  for (int i = 0; i < 3000; ++i) { double p[4] = {10 * frand(&seed), 10 * frand(&seed), 0.0, wp[0] * frand(&seed)}; orc_kd_insert(w, p); }
  for (int k = 0; k < 100; ++k) {
    double q[4] = {10 * frand(&seed), 10 * frand(&seed), 0.0, wp[0] * frand(&seed)};
    orc_list *l = orc_kd_find_within_range(w, 3.5, q);
    int64_t n = orc_list_length(l);
    int64_t m = orc_range_naive(w, 3.5, q, 0, NULL, NULL);
    bad += (n != m);
    orc_kd_empty_range_list(w, l);
    double g[8 * 4];
    (void)orc_ghost_points(w, q, 3.5, 8, g);
  }
  orc_kd_destroy(w);
  /* spheres, polygons, dubins */
  orc_sphere sp[4];
  for (int i = 0; i < 4; ++i) { sp[i].c[0] = 3.0 * i; sp[i].c[1] = 0; sp[i].c[2] = 0; sp[i].radius = 1.0; sp[i].life_span = INFINITY; sp[i].unused = (i == 2); sp[i].pad = 0; }
  double p0[3] = {-2, 1.4, 0}, p1[3] = {2, 1.4, 0}, z[3] = {10, 10, 10};
  int32_t fh;
  bad += orc_edge_check_spheres(sp, 4, p0, p1, 0.5, &fh) != 0;
  bad += orc_edge_check_spheres(sp, 4, z, z, 0.5, &fh) != 1;
  double clr; (void)orc_point_check_spheres(sp, 4, p0, 0.5, 1, &clr);
  double sq[8] = {0, 0, 1, 0, 1, 1, 0, 1};
  orc_polygon pg; pg.kind = 3; pg.nverts = 4; pg.verts = sq; pg.life_span = INFINITY; pg.unused = 0; pg.npath = 0; pg.path = 0;
  orc_polygon_ctor(sq, 4, &pg.cx, &pg.cy, &pg.radius);
  double e0[2] = {-1, .5}, e1[2] = {2, .5};
  bad += orc_edge_check_polygons(&pg, 1, e0, e1, 0.1, &fh) != 1;
  (void)orc_point_check_polygons(&pg, 1, e0, 0.1, &clr);
  /* moving obstacle (kind 6) + k nearest under the sanitizers */
  double mpath[6] = {0, 0, 0, 10, 0, 10};
  orc_polygon mv = pg; mv.kind = 6; mv.npath = 2; mv.path = mpath;
  double m0[3] = {5, -5, 0}, m1[3] = {5, 5, 10}, m2[3] = {5, -5, 20}, m3[3] = {5, 5, 30};
  bad += orc_edge_check_polygons(&mv, 1, m0, m1, 0.1, &fh) != 1;
  bad += orc_edge_check_polygons(&mv, 1, m2, m3, 6.0, &fh) != 0;
  double mp[3] = {5.5, 0.5, 5};
  bad += orc_point_check_polygons(&mv, 1, mp, 0.5, &clr) != 1;
  {
    orc_kd *kt = orc_kd_create(3);
    for (int i = 0; i < 500; ++i) { double p[3] = {frand(&seed), frand(&seed), frand(&seed)}; orc_kd_insert(kt, p); }
    int32_t ki[40]; double kd[40];
    for (int i = 0; i < 50; ++i) {
      double q[3] = {frand(&seed), frand(&seed), frand(&seed)};
      bad += orc_kd_knearest(kt, 1, q, 40, ki, kd) != 2;
      bad += orc_kd_knearest(kt, 33, q, 40, ki, kd) != 33;
      bad += orc_kd_knearest_naive(kt, 7, q, 40, ki, kd) != 7;
    }
    orc_kd_destroy(kt);
  }
  double traj[2 * 1024]; int tl; double cost; char word[4];
  for (int k = 0; k < 2000; ++k) {
    double s[4] = {20 * frand(&seed), 20 * frand(&seed), 0, 6.28 * frand(&seed)};
    double g[4] = {s[0] + 6 * (frand(&seed) - .5), s[1] + 6 * (frand(&seed) - .5), 0, 6.28 * frand(&seed)};
    orc_dubins_steer(s, g, 1.0, &cost, word, traj, 1024, &tl);
    bad += !(cost > 0) || tl > 1024;
    (void)orc_dubins_edge_check_polygons(&pg, 1, s, g, traj, tl, 0.5, 1.0, &fh);
  }
  {
    /* the batched forms: growing trajectory scratch, trajectory CSR, the candidate loop */
    enum { NB = 300 };
    static double bs[4 * NB], bg[4 * NB], bc[NB], bw[NB], bv[NB], brows[3 * 200 * NB], nodes[4 * 50], qs[4 * 6];
    static char bwd[3 * NB];
    static int32_t btl[NB], bfh[NB];
    static uint8_t bh[NB], bok[NB];
    static int64_t boff[NB + 1], coff[7];
    for (int i = 0; i < NB; ++i) {
      double *s = bs + 4 * i, *g = bg + 4 * i;
      s[0] = 20 * frand(&seed); s[1] = 20 * frand(&seed); s[2] = 30; s[3] = 6.28 * frand(&seed);
      g[0] = s[0] + 3 * (frand(&seed) - .5); g[1] = s[1] + 3 * (frand(&seed) - .5); g[2] = 28; g[3] = 6.28 * frand(&seed);
    }
    for (int t3 = 0; t3 < 2; ++t3) {
      bad += orc_dubins_edges_batch(bs, bg, NB, 1.0, 0.5, &pg, 1, t3, t3, 5.0, 30.0, bc, bw, bv, bwd, btl, bh, bfh, bok,
                                    NULL, NULL) != 0;
      boff[0] = 0;
      for (int i = 0; i < NB; ++i) boff[i + 1] = boff[i] + ((i % 3) ? btl[i] : 0);
      bad += orc_dubins_edges_batch(bs, bg, NB, 1.0, 0.5, &pg, 1, t3, 0, 5.0, 30.0, NULL, NULL, NULL, NULL, NULL, NULL,
                                    NULL, NULL, boff, brows) != 0;
    }
    bad += orc_dubins_edges_batch(bs, bg, NB, 1.0, 0.5, &mv, 1, 0, 0, 0, 0, bc, NULL, NULL, NULL, NULL, NULL, NULL, NULL,
                                  NULL, NULL) != -1;
    for (int i = 0; i < 50; ++i) { nodes[4 * i] = 20 * frand(&seed); nodes[4 * i + 1] = 20 * frand(&seed); nodes[4 * i + 2] = 25; nodes[4 * i + 3] = 6.28 * frand(&seed); }
    for (int i = 0; i < 6; ++i) { qs[4 * i] = 20 * frand(&seed); qs[4 * i + 1] = 20 * frand(&seed); qs[4 * i + 2] = 30; qs[4 * i + 3] = 6.28 * frand(&seed); }
    coff[0] = 0;
    for (int i = 0; i < 6; ++i) coff[i + 1] = coff[i] + (i == 2 ? 0 : 40);
    int32_t cidx[200];
    for (int e = 0; e < 200; ++e) cidx[e] = (int32_t)(50 * frand(&seed));
    bad += orc_dubins_candidates_batch(qs, 6, coff, cidx, nodes, 37, 200, 1.0, 0.5, &mv, 1, 1, 1, 5.0, 30.0, bc, bw, bh,
                                       bok, btl, bfh) != 0;
    bad += orc_dubins_candidates_batch(qs, 6, coff, cidx, nodes, 0, 201, 1.0, 0.5, &mv, 1, 1, 1, 5.0, 30.0, bc, bw, bh,
                                       bok, btl, bfh) != -2;
  }
  {
    /* batched search and SimpleEdge checks: capacity retry, per-query radii, a wrapped tree, k nearest */
    enum { NN = 2000, NQ = 40 };
    static double pts[3 * NN], qs3[3 * NQ], rad[NQ], key[64 * NQ * 4], cout_[64 * NQ * 4], cin_[64 * NQ * 4], clr3[NQ];
    static int32_t idx[64 * NQ * 4], fo[64 * NQ * 4], fi[64 * NQ * 4], kcnt[NQ];
    static int64_t off[NQ + 1], nidx[NQ];
    static uint8_t ho[64 * NQ * 4], hi[64 * NQ * 4], uns[NQ];
    static double ndist[NQ];
    orc_kd *bt = orc_kd_create(3);
    for (int i = 0; i < 3 * NN; ++i) pts[i] = frand(&seed);
    orc_kd_insert_many(bt, pts, NN);
    for (int i = 0; i < 3 * NQ; ++i) qs3[i] = frand(&seed);
    for (int i = 0; i < NQ; ++i) rad[i] = (i % 5) ? 0.12 * frand(&seed) : 0.0;
    const int64_t need = orc_range_batch(bt, qs3, NQ, rad, 1, 8, off, idx, key, nidx, ndist);
    bad += !(need > 8) || off[NQ] != need;
    bad += orc_range_batch(bt, qs3, NQ, rad, 1, need, off, idx, key, nidx, ndist) != need;
    for (int i = 0; i < NQ; ++i)
      for (int64_t e = off[i] + 1; e < off[i + 1]; ++e) bad += !(idx[e - 1] < idx[e]);
    bad += orc_range_batch(bt, qs3, NQ, rad, 0, 0, NULL, NULL, NULL, nidx, ndist) != 0;
    bad += orc_simple_candidates_batch(qs3, NQ, 3, off, idx, pts, 3, need, sp, NULL, 4, 0.5, cout_, cin_, ho, hi, fo,
                                       fi) != 0;
    bad += orc_simple_candidates_batch(qs3, NQ, 3, off, idx, pts, 0, need, NULL, &pg, 1, 0.5, cout_, cin_, ho, hi, fo,
                                       fi) != 0;
    bad += orc_simple_candidates_batch(qs3, NQ, 3, off, idx, pts, 0, need + 1, sp, NULL, 4, 0.5, cout_, cin_, ho, hi,
                                       fo, fi) != -2;
    orc_edges_check_batch(pts, pts + 3, NN - 1, 3, sp, NULL, 4, 0.5, ho, fo);
    orc_edges_check_batch(pts, pts + 3, NN - 1, 3, NULL, &mv, 1, 0.5, ho, NULL);
    orc_points_check_batch(qs3, NQ, 3, sp, NULL, 4, 0.5, 1, uns, clr3);
    orc_points_check_batch(qs3, NQ, 3, NULL, &pg, 1, 0.5, 0, uns, NULL);
    bad += orc_knearest_batch(bt, 5, qs3, NQ, 5, idx, key, kcnt) != 0 || kcnt[0] != 5;
    bad += orc_knearest_batch(bt, 1, qs3, NQ, 1, idx, key, kcnt) != -2;
    orc_kd_destroy(bt);
    orc_kd *wt = orc_kd_create(4);
    int wd1[1] = {3}; double wp1[1] = {2.0 * 3.141592653589793};
    orc_kd_set_wraps(wt, 1, wd1, wp1);
    static double pts4[4 * NN], qs4[4 * NQ];
    for (int i = 0; i < NN; ++i) { pts4[4 * i] = 10 * frand(&seed); pts4[4 * i + 1] = 10 * frand(&seed); pts4[4 * i + 2] = 0; pts4[4 * i + 3] = wp1[0] * frand(&seed); }
    for (int i = 0; i < NQ; ++i) { qs4[4 * i] = 10 * frand(&seed); qs4[4 * i + 1] = 10 * frand(&seed); qs4[4 * i + 2] = 0; qs4[4 * i + 3] = wp1[0] * frand(&seed); }
    orc_kd_insert_many(wt, pts4, NN);
    double r4 = 0.6;
    const int64_t need4 = orc_range_batch(wt, qs4, NQ, &r4, 0, 0, off, NULL, NULL, NULL, NULL);
    bad += need4 > 64 * NQ * 4 || orc_range_batch(wt, qs4, NQ, &r4, 0, need4, off, idx, key, nidx, ndist) != need4;
    bad += orc_knearest_batch(wt, 3, qs4, NQ, 3, idx, key, kcnt) != -1;
    orc_kd_destroy(wt);
  }
  {
    /* batched graph forms and the sweep edge loop: every edge kind, add and remove, the argument checks */
    enum { GN = 400, GE = 2400 };
    static int32_t ges[GE], gee[GE];
    static double gw[GE], glmc[GN + 1], gtc[GN + 1], n3[3 * GN], n4[4 * GN], n4t[4 * GN];
    static int64_t gpar[GN + 1], gblk[40];
    static uint8_t mask[GN], sel[GE];
    for (int e = 0; e < GE; ++e) {
      ges[e] = e % GN; gee[e] = (int32_t)((e % GN + 1 + (int)(20 * frand(&seed))) % GN);
      gw[e] = 0.1 + frand(&seed);
    }
    orc_graph *gg = orc_graph_create(GN + 1);
    bad += orc_graph_add_edges(gg, ges, gee, gw, 0, 0, 1) != 0;
    bad += orc_graph_add_edges(gg, ges, gee, gw, GE / 2, 0, 1) != 0;
    bad += orc_graph_add_edges(gg, ges + GE / 2, gee + GE / 2, gw + GE / 2, GE - GE / 2, 1, 1) != GE / 2;
    for (int v = 0; v <= GN; ++v) orc_graph_set_node(gg, v, INFINITY, INFINITY);
    orc_graph_set_node(gg, 0, 0.0, INFINITY);
    orc_graph_verify_in_queue(gg, 0);
    orc_graph_reduce_inconsistency(gg, GN, 0, INFINITY, 0.0);
    orc_graph_read(gg, NULL, NULL, NULL);
    orc_graph_read(gg, glmc, gtc, gpar);
    for (int v = 0; v < GN; ++v) bad += glmc[v] != orc_graph_lmc(gg, v) || gpar[v] != orc_graph_parent_edge(gg, v);
    for (int k = 0; k < 40; ++k) gblk[k] = (k % 2) && gpar[k + 1] >= 0 ? gpar[k + 1] : (int64_t)(GE * frand(&seed));
    orc_graph_block_edges(gg, gblk, 0);
    orc_graph_block_edges(gg, gblk, 40);
    orc_graph_propagate_descendants(gg);
    orc_graph_reduce_inconsistency(gg, GN, 0, INFINITY, 0.0);
    orc_graph_read(gg, glmc, NULL, NULL);
    orc_graph_destroy(gg);
    for (int v = 0; v < GN; ++v) {
      n3[3 * v] = 10 * frand(&seed); n3[3 * v + 1] = 10 * frand(&seed); n3[3 * v + 2] = 0;
      n4[4 * v] = n3[3 * v]; n4[4 * v + 1] = n3[3 * v + 1]; n4[4 * v + 2] = 0; n4[4 * v + 3] = 6.28 * frand(&seed);
      n4t[4 * v] = n4[4 * v]; n4t[4 * v + 1] = n4[4 * v + 1]; n4t[4 * v + 2] = 20 * frand(&seed); n4t[4 * v + 3] = n4[4 * v + 3];
      mask[v] = (uint8_t)(frand(&seed) < 0.6);
    }
    for (int e = 0; e < GE; ++e) gw[e] = (e % 3) ? INFINITY : 1.0;
    orc_polygon two[2] = {pg, pg};
    two[1].verts = sq; two[1].cx += 0.25;
    orc_polygon tmv[2] = {mv, mv};
    tmv[1].unused = 1;
    for (int rm = 0; rm < 2; ++rm) {
      bad += orc_sweep_edges_batch(ges, gee, gw, 5, GE, n3, 3, mask, sp, NULL, 4, 1, rm, ORC_EDGE_SIMPLE, 0.5, 0, sel) != 0;
      bad += orc_sweep_edges_batch(ges, gee, gw, 0, GE, n3, 3, mask, NULL, two, 2, 0, rm, ORC_EDGE_SIMPLE, 0.5, 0, sel) != 0;
      bad += orc_sweep_edges_batch(ges, gee, gw, 0, 300, n4, 4, mask, NULL, two, 2, 1, rm, ORC_EDGE_DUBINS, 0.5, 1.0, sel) != 0;
      bad += orc_sweep_edges_batch(ges, gee, gw, 0, 300, n4t, 4, mask, NULL, tmv, 2, 0, rm, ORC_EDGE_DUBINS_TIME, 0.5, 1.0,
                                   sel) != 0;
    }
    bad += orc_sweep_edges_batch(ges, gee, gw, 0, 300, n4, 4, mask, NULL, tmv, 2, 0, 0, ORC_EDGE_DUBINS, 0.5, 1.0, sel) != -1;
    bad += orc_sweep_edges_batch(ges, gee, gw, 0, 3, n3, 3, mask, sp, NULL, 4, 4, 0, ORC_EDGE_SIMPLE, 0.5, 0, sel) != -2;
    bad += orc_sweep_edges_batch(ges, gee, gw, 0, 3, n4, 4, mask, sp, NULL, 4, 0, 0, ORC_EDGE_DUBINS, 0.5, 1.0, sel) != -2;
    bad += orc_sweep_edges_batch(ges, gee, NULL, 0, 3, n3, 3, mask, sp, NULL, 4, 0, 1, ORC_EDGE_SIMPLE, 0.5, 0, sel) != -2;
    bad += orc_sweep_edges_batch(ges, gee, NULL, 7, 7, n3, 3, mask, sp, NULL, 4, 0, 1, ORC_EDGE_SIMPLE, 0.5, 0, sel) != 0;
  }
  printf(bad ? "selftest FAILED (%d)\n" : "selftest ok\n", bad);
  return bad != 0;
}
