/*
 * rrtx.h -- C ABI of librrtx_hip.so: the MI355X (gfx950) implementation of the
 * RRT^X extend/rewire hot path of jnetter6/RRTQX_3D.
 *
 * The reference (Julia, R/ = code_RRTQx_3D/) has no FFI; the seam is a set of
 * free functions selected by multiple dispatch (R/README.txt:85-99).  Each entry
 * point below names the reference function(s) it replaces.  The Julia binding a
 * maintainer would add is shown in INTEGRATION.md and julia/RRTXHip.jl.
 *
 * Conventions
 *   - plain pointers and sizes only; all host buffers are caller-owned and only
 *     read/written for the duration of the call (GC.@preserve on the Julia side);
 *   - every function returns RRTX_OK (0) or a negative RRTX_E_* code and never
 *     throws or aborts; rrtx_last_error(ctx) gives the message;
 *   - points are passed as n x dim row-major doubles (a Julia dim x n Array);
 *   - node indices are 0-based insertion order (index 0 is the kd-tree root);
 *   - a ctx is bound to ONE GPU and is not thread-safe; distinct ctxs are
 *     independent (one per planner/agent tree, R/rrtqx.jl:29-31);
 *   - all arithmetic is IEEE fp64 without FMA contraction, so neighbour sets and
 *     collision booleans are bit-identical to the reference's CPU path; NaN
 *     inputs are not errors (a zero-length edge is a "hit", R/DRRT_Q.jl:1208);
 *   - host-pointer calls are synchronous; the *_dev calls take DEVICE pointers,
 *     enqueue on the ctx stream and return immediately (rrtx_sync to wait).
 */
#ifndef RRTX_H
#define RRTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRTX_OK 0
#define RRTX_E_INVALID (-1)  /* bad argument */
#define RRTX_E_CAPACITY (-2) /* caller output buffer too small; see `needed` */
#define RRTX_E_DEVICE (-3)   /* HIP runtime error */
#define RRTX_E_NOMEM (-4)
#define RRTX_E_STATE (-5)    /* call not valid in this state (e.g. empty tree) */

typedef struct rrtx_ctx rrtx_ctx;

typedef struct {
  int64_t n_nodes;
  int32_t dim;
  int32_t n_spheres;         /* as set (active + inactive) */
  int32_t n_polygons;
  int32_t n_wraps;
  /* per-kernel-family device time, accumulated while profiling is enabled
   * (HIP events on the ctx stream around every launch of that family) */
  double ms_nn_scan;     int64_t launches_nn_scan;
  double ms_nn_finish;   int64_t launches_nn_finish;
  double ms_nn_nearest;  int64_t launches_nn_nearest;
  double ms_edges;       int64_t launches_edges;
  double ms_points;      int64_t launches_points;
  double ms_dubins;      int64_t launches_dubins;
  /* work counters of the last rrtx_nn_radius* / rrtx_extend_candidates* call */
  int64_t last_pairs;        /* (query copy, node) visits */
  int64_t last_neighbors;    /* sum of k */
  int32_t last_tile_q;       /* query copies that shared one streamed pass of the node arrays */
  int32_t last_scan_units;   /* slab-culled range scan: (tile of last_tile_q copies, 512-node chunk) pairs the
                              * last call streamed; 0 when it streamed every node for every tile */
  /* (round 3, appended) the steering launches of the Dubins edge paths on their own: ms_dubins above then counts
   * the check kernels (and the stand-alone steer / trajectory calls) */
  double ms_dubins_steer; int64_t launches_dubins_steer;
  int64_t last_sweep_candidates;  /* mirrored edges the last rrtx_obstacle_sweep_polygon put through explicitEdgeCheck;
                                   * after rrtx_obstacle_sweep_polygon_batch: the distinct candidate edges of the call's
                                   * groups of 64 entries, summed over the groups; after
                                   * rrtx_obstacle_release_polygon_batch: the same sum over the BLOCKED (dist == Inf)
                                   * candidate edges only */
} rrtx_stats_t;

/* ---- lifetime ------------------------------------------------------------ */
/* replaces KDTree{T}(d, KDdist) + CSpace obstacle list construction
 * (R/kdTree_general.jl:94-112, R/rrtqx.jl:29-31).  dim is 3 (SimpleEdge, 3-D)
 * or 4 ([x y t theta], Dubins).  device = HIP device ordinal. */
int rrtx_create(rrtx_ctx **out, int dim, int device, int64_t node_capacity);
int rrtx_destroy(rrtx_ctx *ctx);
const char *rrtx_last_error(rrtx_ctx *ctx);
/* message of the last failing rrtx_create (no ctx exists then) */
const char *rrtx_create_error(void);
/* run on a caller-provided hipStream_t (e.g. the stream the caller's framework is using); NULL
 * restores the ctx-owned stream */
int rrtx_set_stream(rrtx_ctx *ctx, void *hip_stream);
void *rrtx_get_stream(rrtx_ctx *ctx);
int rrtx_sync(rrtx_ctx *ctx);
/* per-kernel-family HIP-event timing (resets the sums): 0 = off, 1 = only the range-scan kernel
 * (two event records per call), 2 = every family (each record costs ~10 us between kernels) */
int rrtx_profile(rrtx_ctx *ctx, int enable);
int rrtx_stats(rrtx_ctx *ctx, rrtx_stats_t *out);
/* tuning switches; none of them changes a result.
 *   RRTX_OPT_NN_FILTER (default 1): range search screens (query, node) pairs with a
 *   conservative fp32 bound before the exact unfused fp64 test; 0 = exact test on
 *   every pair. */
#define RRTX_OPT_NN_FILTER 1
/*   RRTX_OPT_SCAN_BLOCKS: target workgroup count of the range scan (launch geometry);
 *   RRTX_OPT_SCAN_TILE_Q: query copies per workgroup tile, 0 = default. */
#define RRTX_OPT_SCAN_BLOCKS 2
#define RRTX_OPT_SCAN_TILE_Q 3
#define RRTX_OPT_SCAN_ITEMS 4  /* target number of (tile, node segment) work items */
/*   RRTX_OPT_NN_CULL (default 1): the range search keeps a second copy of the node shadow
 *   ordered by (x, y) grid cell and buckets each call's query copies by cell, so a tile of
 *   copies only streams the 512-node chunks whose x/y extent can reach it.  Purely a skip of
 *   pairs that provably fail the exact test; results are identical.  0 = off (every tile
 *   streams every node), 1 = on for trees of at least 8192 nodes, 2 = always on. */
#define RRTX_OPT_NN_CULL 5
/*   RRTX_OPT_PROFILE_EVERY (default 1): with rrtx_profile level 1, only every n-th launch of the
 *   range-search kernel is bracketed by HIP events (an event record between two kernels drains the
 *   pipeline for several microseconds); rrtx_stats then reports the timed launches only. */
#define RRTX_OPT_PROFILE_EVERY 6
/*   RRTX_OPT_KNN_LISTS (default 1): rrtx_nn_knearest takes the k nearest of a query from its
 *   range-search list (radius guessed from a sample of the batch) and runs the exhaustive
 *   selection kernel only for queries whose list holds fewer than k nodes; 0 = exhaustive for all. */
#define RRTX_OPT_KNN_LISTS 7
/*   RRTX_OPT_EXTEND_OBSTACLES (default 0): which obstacle list rrtx_extend_candidates* checks the
 *   candidate edges and the samples against -- 0 = the sphere list (explicitEdgeCheck3D, the 3-D
 *   planner of R/rrtqx.jl), 1 = the polygon list (explicitEdgeCheck2D on the (x, y) projection and the
 *   polygon explicitPointCheck, R/DRRT.jl:1434-1470, 1523-1678; time in the third coordinate for the
 *   moving kinds).  This one DOES select behaviour: it says which CSpace.obstacles the caller has. */
#define RRTX_OPT_EXTEND_OBSTACLES 8
/*   RRTX_OPT_NEAREST_REC_CAP (testing, default 0 = sized from the batch): candidate records the screened
 *   nearest scan may keep; queries that lose one are answered again exactly on the device. */
#define RRTX_OPT_NEAREST_REC_CAP 9
/*   RRTX_OPT_BUCKET_MULT (default 2, grows by itself after a call whose lists overflowed): capacity of the
 *   per-query hit buckets of the range search in units of cap / nq; 2, 4, 8 or 16. */
#define RRTX_OPT_BUCKET_MULT 10
/*   RRTX_OPT_TUNE (default 0): bit mask of kernel variants under measurement; results are identical.  Bit 4:
 *   the culled range search without ghosts keeps the place pass (RRTX_OPT_LAST_PLACEMENT).  Value 8 (bit 3): the tile
 *   kernel of the culled range search keeps its looped form where the straight one would run
 *   (rrtx_last_tile_form). */
#define RRTX_OPT_TUNE 11
/*   RRTX_OPT_SPACE_HAS_TIME (default 0; dim = 4 only): CSpace.spaceHasTime (R/DRRT_data_structures.jl:330) for the
 *   Dubins entry points.  The third coordinate of [x y t theta] is then time (planning runs in reverse time:
 *   an edge's start node is LATER than its end node): edge.dist = sqrt(Wdist^2 + dt^2), edge.velocity =
 *   Wdist / dt and edge.trajectory carries a time column (R/DRRT_DubinsEdge_functions.jl:660-697), validMove
 *   wants start time > end time and a velocity within rrtx_set_dubins_velocity's bounds (:115-121), and the two-stage
 *   edge check hands its chord and its pieces to explicitEdgeCheck2D with their times, so polygons that move
 *   in time (kinds 6 / 7) are tested where they are when the robot passes (:750-774, R/DRRT.jl:1579-1651).
 *   This one DOES select behaviour: it says which space the caller plans in. */
#define RRTX_OPT_SPACE_HAS_TIME 12
/*   RRTX_OPT_ROOT_RULE (default 1): node 0 of this context is the kd-tree's root, which the range search takes
 *   with <= (R/kdTree_general.jl:896).  0 for a context that holds a LATER index range of a tree sharded over
 *   several GPUs (rrtqx_3d_amd/parallel.py): its node 0 is an ordinary node. */
#define RRTX_OPT_ROOT_RULE 13
/*   RRTX_OPT_LAST_PLACEMENT (read only): how the last range search ordered its query copies -- 0 no culling (no
 *   order), 1 the place pass (ghosts, or RRTX_OPT_TUNE bit 4), 2 the tile kernel from the bucket-slot table. */
#define RRTX_OPT_LAST_PLACEMENT 14
/*   RRTX_OPT_SELECT_LIST_CAP: entries the context-owned neighbour lists of rrtx_extend_select have room for.  The call
 *   sizes them itself (from what the last calls produced; a call that produces more grows them and runs once more);
 *   reading tells what it settled on, setting forces a starting value (testing). */
#define RRTX_OPT_SELECT_LIST_CAP 15
/*   RRTX_OPT_DUBINS_TIME_COLUMN (default RRTX_TIME_COLUMN_PIECEWISE; any value but the two below is RRTX_E_INVALID):
 *   how the time column of a Dubins edge's stored polyline is formed in a dim = 4 context with
 *   RRTX_OPT_SPACE_HAS_TIME (without it the option has no effect).  Let rows 0 .. P-1 be the stored rows before the
 *   last one is overwritten with the end node, st the start node's time and vel = Wdist / (st - end time).
 *     RRTX_TIME_COLUMN_PIECEWISE: the distance walked at row k of a piece is (distance at the piece's first row) +
 *       k x (the piece's first chord), the three junctions measured once.  Differs from the reference by rounding.
 *     RRTX_TIME_COLUMN_RUNNING_SUM: the reference's own column (R/DRRT_DubinsEdge_functions.jl:689-695):
 *       cum_0 = 0, cum_i = fl(cum_{i-1} + len(row_{i-1}, row_i)) for i = 1 .. P-2, strictly left to right, with
 *       len = sqrt((dx * dx) + (dy * dy)) unfused and correctly rounded; t_i = st - cum_i / vel.
 *   In both forms row 0 carries st and row P-1 is the end node's (x, y, t).  Costs, words, velocities, validMove, row
 *   counts and the (x, y) of every row do not depend on the option.  Every consumer of the stamps follows it:
 *   rrtx_dubins_trajectory, rrtx_dubins_edges_check, rrtx_dubins_edges_check_obstacle,
 *   rrtx_extend_candidates_dubins(_dev), rrtx_find_new_target_dubins and the Dubins branch of
 *   rrtx_obstacle_sweep_polygon.  This one DOES select behaviour (in the last bits of the stamps). */
#define RRTX_OPT_DUBINS_TIME_COLUMN 16
#define RRTX_TIME_COLUMN_PIECEWISE 0
#define RRTX_TIME_COLUMN_RUNNING_SUM 1
int rrtx_set_option(rrtx_ctx *ctx, int option, int64_t value);
/* The value an option currently has (as rrtx_set_option normalised it): callers that size buffers by an
 * option -- the row width of rrtx_dubins_trajectory -- read it here instead of keeping a shadow copy. */
int rrtx_get_option(rrtx_ctx *ctx, int option, int64_t *value);
/* The form of the tile kernel in the last range search (read only, a fact about the last call and no option):
 * 0 no tile kernel (no culling), 1 looped (a workgroup walks several tiles: more than 4096 (tile, part) pairs, i.e.
 * batches beyond 65 536 copies; or several chunk passes: trees beyond 524 288 nodes; or RRTX_OPT_TUNE value 8),
 * 2 straight (one tile and one chunk pass per workgroup, compiled without the two loops).  Both forms give the same
 * lists. */
int rrtx_last_tile_form(rrtx_ctx *ctx, int *form);
/* Host-pointer entry points move their results through a pinned staging arena owned by the context (DMA at PCIe rate,
 * then one memcpy per output array).  A caller that keeps its output arrays alive across calls -- the Julia host
 * preallocates them -- can have them page-locked instead: after rrtx_host_register(ptr, bytes) every output pointer
 * inside [ptr, ptr + bytes) receives its DMA directly (hipHostRegister; unregister before freeing the array).
 * Results are identical either way. */
int rrtx_host_register(rrtx_ctx *ctx, void *ptr, size_t bytes);
int rrtx_host_unregister(rrtx_ctx *ctx, void *ptr);

/* Host-only helper (no GPU needed): the exact thresholds on SQUARED distances the kernels
 * compare against, so that no device sqrt sits on a decision path:
 *   *first_ge = min{ s >= 0 : sqrt(s) >= r }   (sqrt(s) <  r  <=>  s < *first_ge)
 *   *first_gt = min{ s >= 0 : sqrt(s) >  r }   (sqrt(s) <= r  <=>  s < *first_gt)
 * (NaN when no such s exists).  Exposed for testing the host logic. */
int rrtx_sq_thresholds(double r, double *first_ge, double *first_gt);

/* ---- tree (A2, A5) --------------------------------------------------------- */
/* kdInsert (R/kdTree_general.jl:121-170): appends n nodes; *first_index receives
 * the index of the first one (== treeSize before the call). */
int rrtx_nodes_append(rrtx_ctx *ctx, const double *pos, int64_t n, int64_t *first_index);
int64_t rrtx_nodes_count(rrtx_ctx *ctx);
/* device-to-device variant: pos is a device pointer */
int rrtx_nodes_append_dev(rrtx_ctx *ctx, const double *pos_dev, int64_t n);
/* KDTree(d, f, wraps, wrapPoints) (R/kdTree_general.jl:108): dimension
 * dim_index (0-based) wraps with the given period (Dubins theta: 3, 2*pi;
 * R/DRRT.jl:3312).  At most 3 wrapped dimensions. */
int rrtx_set_wrap(rrtx_ctx *ctx, int dim_index, double period);

/* ---- obstacles (A15) ------------------------------------------------------- */
/* CSpace.obstacles as List{SphereObstacle} in LIST ORDER (front first,
 * R/list.jl:53-58).  cxyzr is m x 4; active[i] = !(obstacleUnused || lifeSpan<=0)
 * (R/DRRT_Q.jl:1777); NULL = all active. */
int rrtx_spheres_set(rrtx_ctx *ctx, const double *cxyzr, const uint8_t *active, int m);
/* polygon Obstacles (legacy 2-D path, R/DRRT_data_structures.jl:135-265), list
 * order.  vert_off is m+1 CSR offsets into vxy (2 doubles per vertex);
 * centre_radius is m x 3 (the Obstacle(3, polygon) ctor values, :229-241, or
 * NULL to have the library apply that ctor); kind[i] is 1 (ball), 3 (polygon), or 6 / 7 (polygon
 * moving in time along a path, :140-143; give the paths with rrtx_polygon_paths_set).  Kinds 2, 4
 * and 5 raise or cannot be constructed in the reference (R/DRRT.jl:1546, data_structures:256) and
 * are refused. */
int rrtx_polygons_set(rrtx_ctx *ctx, const int32_t *vert_off, const double *vxy,
                      const double *centre_radius, const uint8_t *kind, const uint8_t *active, int m);
/* Obstacle.path of the moving kinds 6 and 7 (R/DRRT_data_structures.jl:184-187; read by
 * readTimeObstaclesFromfile, R/DRRT_Q.jl:1022-1061): path_off is m+1 CSR row offsets into path_xyt,
 * 3 doubles per row (dx, dy, t) = offset of the obstacle from its ctor position at time t, t
 * ascending; m is the count last given to rrtx_polygons_set (which clears all paths); static kinds
 * have empty ranges.  For kind 7 this is the path the robot currently assumes -- call again after
 * the host recomputed it (changeObstacleDirection, R/DRRT.jl:370-443).  With such obstacles in the
 * list, rrtx_edges_check* / rrtx_points_check* read TIME from the third coordinate of their points
 * (startPoint[3], R/DRRT_Q.jl:1703; point[3], :1369): edges are tested at the closest approach of
 * the two centres against the bounding circle (:1699-1771), points against the polygon moved to its
 * place at that time (R/DRRT.jl:1289-1305, 1395-1420).  A moving obstacle without a path, and Dubins
 * edge checks against moving obstacles in a space WITHOUT time (their pieces carry no time stamp; see
 * RRTX_OPT_SPACE_HAS_TIME), fail with RRTX_E_STATE. */
int rrtx_polygon_paths_set(rrtx_ctx *ctx, const int32_t *path_off, const double *path_xyt, int m);
/* The in-use flag (!obstacleUnused) of k list positions of rrtx_polygons_set: what removeObstacle clears once its loop
 * is over (R/DRRT.jl:3287) and what the discovery of an obstacle sets before its sweep.  active[j] != 0 = obstacles[j] is
 * in use.  Vertices, kinds, centres, radii and paths are kept; everything rrtx_polygons_set derives from the flags (the
 * packed device tables) is derived again at the next call that needs it.  A position outside the list is
 * RRTX_E_INVALID and nothing changes; for a position given twice the last value wins; k == 0 is RRTX_OK. */
int rrtx_polygons_set_active(rrtx_ctx *ctx, const int32_t *obstacles, int k, const uint8_t *active /* k */);
/* obstacleAugmentation / expiry (R/obstacleAugmentation.jl:106-114,
 * R/DRRT_Q.jl:3301): change radius and/or active flag of sphere `which`. */
int rrtx_obstacle_update(rrtx_ctx *ctx, int which, double radius, uint8_t active);

/* ---- nearest neighbours (A3, A4) ------------------------------------------ */
/* kdFindNearest (R/kdTree_general.jl:357-385), batched.  idx/dist: nq entries.
 * Ties on distance resolve to the lowest index (the reference's tie order is
 * its tree-visit order). */
int rrtx_nn_nearest(rrtx_ctx *ctx, const double *q, int nq, int32_t *idx, double *dist);
/* kdFindKNearest (R/kdTree_general.jl:696-723; helpers :580-593, :605-692), batched.  The
 * reference seeds its heap with the root and an Inf-keyed dummy, so it hands back max(k, 2)
 * nodes (fewer when the tree is smaller): rows of idx/dist are max(k, 2) wide, count[i] says
 * how many entries of row i are filled (unused slots: idx -1, dist +Inf).  Rows come sorted by
 * ascending (distance, index) -- the reference returns heap order -- and ties at the last place
 * go to the lowest indices.  Nodes at a non-finite distance are never returned.  1 <= k <= 2048.
 * Like the reference (:711-713) the call fails on a wrapped space (RRTX_E_STATE).  The reference
 * itself never calls this search (RRT^X uses the radius search).  See RRTX_OPT_KNN_LISTS. */
int rrtx_nn_knearest(rrtx_ctx *ctx, const double *q, int nq, int k, int32_t *idx, double *dist, int32_t *count);
/* kdFindWithinRange (R/kdTree_general.jl:889-919), batched: for query i the
 * nodes with KDdist < r[i] (the root, index 0, with <=), wrapped dimensions
 * handled with the reference's ghost rule; each list sorted by node index,
 * dist = the key the reference stores.  CSR output; if the total exceeds cap
 * the call returns RRTX_E_CAPACITY with *needed set (offsets are still valid).
 * r_stride: 0 = one radius r[0] for all queries, 1 = r[i] per query. */
int rrtx_nn_radius(rrtx_ctx *ctx, const double *q, const double *r, int r_stride, int nq,
                   int64_t *offsets /* nq+1 */, int32_t *idx, double *dist, int64_t cap,
                   int64_t *needed);

/* ---- collision (A8-A12) ----------------------------------------------------- */
/* explicitEdgeCheck(C, edge) (R/DRRT_Q.jl:1802-1826) for ne straight edges
 * p0[i] -> p1[i]; obstacle_or_minus1 >= 0 restricts the test to that one
 * obstacle (explicitEdgeCheck(S, edge, ob), R/DRRT_Q.jl:3248).  kind selects
 * the obstacle list: 0 = spheres (explicitEdgeCheck3D, :1775-1795, uses the
 * first 3 coordinates), 1 = polygons (explicitEdgeCheck2D, R/DRRT.jl:1523-1578,
 * uses the first 2).  hit[i] in {0,1}; first_hit[i] = list position of the
 * first colliding obstacle or -1 (may be NULL). */
int rrtx_edges_check(rrtx_ctx *ctx, int kind, const double *p0, const double *p1, int64_t ne,
                     double robot_radius, int obstacle_or_minus1, uint8_t *hit, int32_t *first_hit);
/* The same test for edges given as NODE INDEX pairs (the planner's graph edges), as the obstacle
 * sweeps need it: addNewObstacle tests every out-edge of the nodes near a new obstacle against
 * that one obstacle (R/DRRT_Q.jl:3220-3290: obstacle_or_minus1 = its list position); removeObstacle
 * re-tests freed edges against the OTHER obstacles that are active in their time window
 * (R/DRRT_Q.jl:3321-3337: obstacle_mask[i] != 0 selects them; NULL = all).  Sphere list only. */
int rrtx_edges_check_idx(rrtx_ctx *ctx, const int32_t *start_idx, const int32_t *end_idx, int64_t ne,
                         double robot_radius, int obstacle_or_minus1, const uint8_t *obstacle_mask,
                         uint8_t *hit, int32_t *first_hit);
/* Obstacle sweep against a device mirror of the planner's directed edges.
 * rrtx_graph_edges_append registers edges start -> end (node indices; what RRTNodeNeighborIterator
 * walks: the out-neighbour edges and the parent edge of every node) and returns the id of the first
 * one; ids are consecutive.  The sweeps and releases tolerate a mirror that is a superset of the live graph (they
 * only list ids, and the caller ignores those of edges it has dropped); the cost propagation does not, so the edges
 * the planner culls are dropped on the device with rrtx_graph_edges_cull and removed with rrtx_graph_edges_compact
 * (below, after rrtx_graph_cost_update_delta).  rrtx_obstacle_sweep is the edge loop of addNewObstacle
 * (R/DRRT_Q.jl:3195-3290): nodes within search_range (= robotRadius + delta + ob.radius) of sphere
 * `obstacle`'s centre -- kdFindWithinRange, root with <= -- and, among the registered edges that
 * START at such a node, those for which explicitEdgeCheck(S, edge, ob) is true.  edge_ids receives
 * their ids in ascending order (two-call capacity pattern).  An inactive obstacle collides with
 * nothing (R/DRRT_Q.jl:1777). */
int rrtx_graph_edges_append(rrtx_ctx *ctx, const int32_t *start_idx, const int32_t *end_idx, int64_t n,
                            int64_t *first_id);
int64_t rrtx_graph_edges_count(rrtx_ctx *ctx);
int rrtx_graph_edges_clear(rrtx_ctx *ctx);
int rrtx_obstacle_sweep(rrtx_ctx *ctx, int obstacle, double search_range, double robot_radius, int32_t *edge_ids,
                        int64_t cap, int64_t *needed);
/* rrtx_obstacle_sweep for k sphere obstacles in one pass over the mirror: the edge loops of a burst of addNewObstacle
 * calls (R/DRRT_Q.jl:3195-3290 each) -- the obstacles another agent injects in one main-loop iteration, or every
 * active obstacle re-added when the kino-distance grows.  obstacles[j] is a list position of rrtx_spheres_set,
 * search_range[j] its range (= robotRadius + delta + radius).  CSR output: row j, edge_ids[offsets[j] .. offsets[j+1]),
 * is exactly what rrtx_obstacle_sweep(ctx, obstacles[j], search_range[j], robot_radius, ...) returns -- the same ids,
 * ascending; the thresholds of every obstacle are the ones that call computes.  Rows come in the order of
 * `obstacles`; an edge that collides with several obstacles is in each of their rows; an obstacle that is not in use
 * gives an empty row (R/DRRT_Q.jl:1777); a position listed twice gives two equal rows.
 *   0 <= k <= 65536; k == 0 is RRTX_OK with offsets[0] = 0.  A position outside the sphere list is RRTX_E_INVALID and
 *   nothing runs.  An empty tree and dim != 3 are RRTX_E_STATE, as in the single call; an empty mirror gives empty rows.
 *   Two-call capacity pattern: with more than cap ids in all rows together the call returns RRTX_E_CAPACITY with
 *   *needed set and offsets valid.
 *   block != 0: after a call that returns RRTX_OK every returned edge is blocked in the mirror, on the device, exactly
 *   as rrtx_graph_edges_block over the union of the rows leaves it (dist = Inf, marked as touched for the next
 *   rrtx_graph_cost_update); the ids do not travel down and up again for it.  A call that does not return RRTX_OK
 *   blocks nothing.  Blocking never changes what this or a later sweep returns: the sphere sweep does not read dist. */
int rrtx_obstacle_sweep_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, const double *search_range /* k */,
                              double robot_radius, int block, int64_t *offsets /* k + 1 */, int32_t *edge_ids,
                              int64_t cap, int64_t *needed);
/* The leaving half: the edge loops of a burst of CORRECTED removeObstacle calls (R/DRRT_Q.jl:3295-3362 each) in one pass
 * over the mirror -- the expired spheres of one main-loop iteration.  The reference marks the obstacle unused before its
 * edge loop (R/DRRT_Q.jl:3302) and an unused obstacle collides with nothing (R/DRRT_Q.jl:1777), so as written that loop
 * never frees an edge; this call is what the loop means.  The call says which obstacles leave, the list's flags say
 * which stay: with L the set of positions in `obstacles`, sphere i STAYS when active[i] (as last given to
 * rrtx_spheres_set / rrtx_obstacle_update) and i is not in L.  CSR output as in rrtx_obstacle_sweep_batch: row j,
 * edge_ids[offsets[j] .. offsets[j+1]), holds in ascending order the ids e for which all of
 *   1. dist[e] == +Inf in the mirror when the call starts (the edge is blocked);
 *   2. the start node of e is within search_range[j] (= robotRadius + delta + radius) of the centre of sphere
 *      obstacles[j] -- the thresholds of rrtx_obstacle_sweep, the root taken with <=;
 *   3. explicitEdgeCheck(S, e, sphere obstacles[j]) with the sphere inflated by robot_radius.  THE FLAG OF obstacles[j]
 *      ITSELF IS NOT READ: a caller that follows the reference's order (mark unused at :3302, then loop) and one that
 *      clears the flag afterwards get the same rows;
 *   4. explicitEdgeCheck(S, e, sphere i) holds for no sphere i that stays
 * hold.  An edge is in the row of every leaving obstacle it satisfies 1-3 for; test 4 is the same for every row; every
 * row sees the mirror as it stood at entry; a position listed twice gives two equal rows.  The time-window condition
 * of :3326-3337 (startTime <= timeElapsed <= startTime + lifeSpan of the others) is folded into the flags by the
 * caller, as for rrtx_obstacle_sweep_polygon mode 1.
 *   0 <= k <= 65536; k == 0 is RRTX_OK with offsets[0] = 0.  A position outside the sphere list is RRTX_E_INVALID and
 *   nothing runs.  An empty tree and dim != 3 are RRTX_E_STATE; an empty mirror gives empty rows.  Two-call capacity
 *   pattern: with more than cap ids in all rows together the call returns RRTX_E_CAPACITY with *needed set and
 *   offsets valid.
 *   unblock != 0: after a call that returns RRTX_OK every returned edge is left, on the device, exactly as
 *   rrtx_graph_edges_unblock over the union of the rows leaves it (dist = distOriginal, R/DRRT_Q.jl:3342, marked as
 *   touched for the next rrtx_graph_cost_update); the ids do not travel down and up again for it.  A call that does
 *   not return RRTX_OK unblocks nothing. */
int rrtx_obstacle_release_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, const double *search_range /* k */,
                                double robot_radius, int unblock, int64_t *offsets /* k + 1 */, int32_t *edge_ids,
                                int64_t cap, int64_t *needed);
/* The obstacle sweeps of the POLYGON list -- the 2-D Euclidean and the Dubins space, with or without time
 * (legacy planner, R/DRRT.jl:3048-3290; BASELINE config 5's "dynamic discoverable obstacles" run these).  The edge
 * type is the context's: dim = 3 SimpleEdge, dim = 4 DubinsEdge (r_min = S.minTurningRadius; with
 * RRTX_OPT_SPACE_HAS_TIME the pieces carry time).  `obstacle` is a list position of rrtx_polygons_set.
 *   nodes: findPointsInConflictWithObstacle (:3048-3125) -- static kinds: range robotRadius + delta + ob.radius
 *     around ob.position (Dubins space: around [x y 0.0 pi] with range + pi; a dim = 3 tree is the 2-D space at
 *     z = 0); kinds 6 / 7: one query per path segment at [ob.position 0.0] + (path[i] + path[i+1]) / 2 with range +
 *     half the segment's length, accumulated (kdFindMoreWithinRange); the root with <=, ghosts of wrapped dimensions
 *     as the range search takes them.  A static obstacle in a space with time is the reference's
 *     error("this type of obstacle not coded for this type of space") -> RRTX_E_STATE;
 *   mode 0, addNewObstacle's loop (:3127-3200): the mirrored edges that START at such a node (its out-neighbour
 *     edges and parent edge) for which explicitEdgeCheck(S, edge, ob) is true -- the caller sets their dist = Inf
 *     (rrtx_graph_edges_block);
 *   mode 1, removeObstacle's loop (:3202-3290): of those edges the ones that are blocked in the mirror
 *     (dist == Inf), collide with ob, and with no OTHER obstacle that is in use -- the caller resets them to
 *     distOriginal (the reference also asks startTime <= timeElapsed <= startTime + lifeSpan of the others: fold
 *     it into their `active` flags).  ob itself must still be in use, as it is in the reference until the loop
 *     is over (:3287); an obstacle not in use collides with nothing and the sweep returns no edge.
 * edge_ids: ascending, two-call capacity pattern (RRTX_E_CAPACITY with *needed set). */
int rrtx_obstacle_sweep_polygon(rrtx_ctx *ctx, int obstacle, double robot_radius, double delta, double r_min, int mode,
                                int32_t *edge_ids, int64_t cap, int64_t *needed);
/* The appearing half for a BURST of polygon obstacles -- the polygons a robot discovers in one main-loop iteration, for
 * each of which the reference runs addNewObstacle before a single reduceInconsistency: mode 0 of
 * rrtx_obstacle_sweep_polygon for k list positions in one call (node query R/DRRT.jl:3048-3125, edge loop
 * R/DRRT.jl:3127-3200).  obstacles[j] is a list position of rrtx_polygons_set.  CSR output: row j is
 * edge_ids[offsets[j] .. offsets[j+1]) and holds exactly what rrtx_obstacle_sweep_polygon(ctx, obstacles[j], robot_radius,
 * delta, r_min, 0, ...) returns -- the same ids, ascending; rows come in the order of `obstacles`.  An edge that collides
 * with several listed obstacles is in each of their rows; an obstacle not in use gives an empty row (R/DRRT.jl:1525); a
 * position listed twice gives two equal rows.  The edge type is the context's, as in the single call: dim = 3 SimpleEdge
 * at z = 0, dim = 4 DubinsEdge with r_min; wraps, RRTX_OPT_SPACE_HAS_TIME, RRTX_OPT_DUBINS_TIME_COLUMN and
 * RRTX_OPT_ROOT_RULE are honoured exactly as the single call honours them.  No row sees another's blocking: every row
 * sees the mirror as it stood at entry (mode 0 does not read dist at all).
 *   Arguments and state: 0 <= k <= 65536; k == 0 is RRTX_OK with offsets[0] = 0.  A NULL offsets, k > 0 with NULL
 *   obstacles, cap < 0 and cap > 0 with NULL edge_ids are RRTX_E_INVALID; a position outside the list is RRTX_E_INVALID
 *   and nothing runs.  An empty tree is RRTX_E_STATE.
 *   Per-obstacle refusals: every listed obstacle is validated before anything runs, in the order j = 0 .. k-1, with the
 *   single call's rules and messages -- a static kind in a space with time (R/DRRT.jl:3067), a moving kind without a
 *   path and a kind that is not coded are RRTX_E_STATE; the `active` flag is not consulted for these checks (nor does
 *   the single call consult it); the first obstacle that would be refused fails the whole call.  DIFFERENCE from the
 *   single call: a dim = 4 context whose list holds a moving kind in use while RRTX_OPT_SPACE_HAS_TIME is off is refused
 *   up front (RRTX_E_STATE, the message of the Dubins edge checks), whatever the mirror holds; the single call only
 *   notices once it has a candidate edge to check.
 *   An empty mirror gives k empty rows (k + 1 zero offsets).
 *   Two-call capacity pattern: with more than cap ids in all rows together the call returns RRTX_E_CAPACITY with *needed
 *   set and offsets valid.
 *   block != 0: after a call that returns RRTX_OK every returned edge is left exactly as rrtx_graph_edges_block over the
 *   union of the rows leaves it (dist = Inf, marked as touched for the next rrtx_graph_cost_update), on the device: the
 *   ids make no round trip for it.  A call that does not return RRTX_OK blocks nothing.  Blocking never changes what this
 *   or a later mode-0 sweep returns: mode 0 does not read dist.
 *   rrtx_stats_t.last_sweep_candidates: the entries are taken in groups of 64 in the order given; a group's candidates
 *   are the mirrored edges that start at a node some obstacle of the group is in conflict with, each counted once; the
 *   field holds their sum over the groups (for k == 1 the single call's number). */
int rrtx_obstacle_sweep_polygon_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, double robot_radius, double delta,
                                      double r_min, int block, int64_t *offsets /* k + 1 */, int32_t *edge_ids,
                                      int64_t cap, int64_t *needed);
/* The leaving half for a BURST of polygon obstacles -- the time-limited polygons that expire in one main-loop iteration
 * (BASELINE config 5), for each of which the reference runs removeObstacle before a single reduceInconsistency: the edge
 * loops of those calls (node query R/DRRT.jl:3048-3125, edge loop R/DRRT.jl:3202-3290) in one call, the members of the
 * burst taken as gone together.  The call says which obstacles leave, the list's flags say which stay: with L the set of
 * list positions in `obstacles`, polygon i STAYS when it is in use (active[i] as last given to rrtx_polygons_set /
 * rrtx_polygons_set_active) and i is not in L.  CSR output as in rrtx_obstacle_sweep_polygon_batch: row j,
 * edge_ids[offsets[j] .. offsets[j+1]), holds in ascending order the mirrored edges e for which all of
 *   1. dist[e] == +Inf in the mirror when the call starts (the edge is blocked);
 *   2. e starts at a node of findPointsInConflictWithObstacle for obstacles[j] -- queries, ghosts, root rule and
 *      thresholds exactly those of rrtx_obstacle_sweep_polygon;
 *   3. explicitEdgeCheck(S, e, obstacles[j]) is true.  The edge type is the context's: dim = 3 SimpleEdge at z = 0,
 *      dim = 4 DubinsEdge with r_min; wraps, RRTX_OPT_SPACE_HAS_TIME, RRTX_OPT_DUBINS_TIME_COLUMN and RRTX_OPT_ROOT_RULE
 *      are honoured exactly as the single call honours them;
 *   4. explicitEdgeCheck(S, e, i) is true for no polygon i that stays
 * hold.  THE FLAG OF obstacles[j] ITSELF IS READ (this differs from rrtx_obstacle_release_batch): the polygon reference
 * keeps the obstacle in use until its loop is over (R/DRRT.jl:3287), so a listed obstacle that is not in use gives an
 * empty row -- and does not stay.  Clear the flags afterwards with rrtx_polygons_set_active.  An edge is in the row of
 * every leaving obstacle it satisfies 1-3 for; test 4 is the same for every row; every row sees the mirror as it stood
 * at entry; a position listed twice gives two equal rows.  Equivalently: row j is what rrtx_obstacle_sweep_polygon(ctx',
 * obstacles[j], robot_radius, delta, r_min, 1, ...) returns on a context ctx' whose OTHER members of L are not in use.
 * The time-window condition of the reference (startTime <= timeElapsed <= startTime + lifeSpan of the others) is folded
 * into the flags by the caller, as for mode 1 of the single call.
 *   Relation to the reference's sequence (remove A, unblock, mark A unused, remove B, ...): while A is removed B still
 *   counts as in use, so an edge blocked by both is freed at B's turn -- provided its start node is in B's node list.
 *   The union of the sequence's rows is therefore always a SUBSET of the union of this call's rows, and the two are
 *   EQUAL when no mirrored edge is longer than delta, which is the planner's invariant (an edge no longer than delta
 *   that collides with B starts within robotRadius + delta + B.radius of B's centre).
 *   Arguments and state, exactly as in rrtx_obstacle_sweep_polygon_batch: 0 <= k <= 65536; k == 0 is RRTX_OK with
 *   offsets[0] = 0.  A NULL offsets, k > 0 with NULL obstacles, cap < 0 and cap > 0 with NULL edge_ids are
 *   RRTX_E_INVALID; a position outside the list is RRTX_E_INVALID and nothing runs.  An empty tree is RRTX_E_STATE.
 *   Every listed obstacle is validated before anything runs, in the order j = 0 .. k-1, with the single call's rules and
 *   messages (RRTX_E_STATE); a dim = 4 context whose list holds a moving kind in use while RRTX_OPT_SPACE_HAS_TIME is off
 *   is refused up front (RRTX_E_STATE).  An empty mirror gives k empty rows (k + 1 zero offsets).
 *   Two-call capacity pattern: with more than cap ids in all rows together the call returns RRTX_E_CAPACITY with *needed
 *   set and offsets valid.
 *   unblock != 0: after a call that returns RRTX_OK every returned edge is left, on the device, exactly as
 *   rrtx_graph_edges_unblock over the union of the rows leaves it (dist = distOriginal, marked as touched for the next
 *   rrtx_graph_cost_update); the ids make no round trip for it.  A call that does not return RRTX_OK unblocks nothing.
 *   rrtx_stats_t.last_sweep_candidates: the entries are taken in groups of 64 in the order given; a group's candidates
 *   are the BLOCKED mirrored edges that start at a node some in-use obstacle of the group is in conflict with, each
 *   counted once; the field holds their sum over the groups. */
int rrtx_obstacle_release_polygon_batch(rrtx_ctx *ctx, const int32_t *obstacles, int k, double robot_radius, double delta,
                                        double r_min, int unblock, int64_t *offsets /* k + 1 */, int32_t *edge_ids,
                                        int64_t cap, int64_t *needed);
/* Cost propagation over the edge mirror: the fixed point that rewire / reduceInconsistency /
 * propogateDescendants (R/DRRT_Q.jl:2490-2541, 2647-2817) drive rrtLMC to when changeThresh = 0 and the queue
 * runs dry -- lmc(root) = 0, lmc(v) = min over mirrored edges v -> u with finite dist of lmc(u) + dist (one
 * rounded addition per edge, the value the reference's heap order also ends at), Inf for a node that cannot
 * reach the root (an orphan).  Every mirrored edge carries edge.dist: the SimpleEdge cost of its two nodes when
 * appended, overwritten with rrtx_graph_edges_set_dist (Dubins costs, costs in a space with time), set to Inf
 * with rrtx_graph_edges_block for the ids rrtx_obstacle_sweep returned (addNewObstacle: `dist = Inf`,
 * R/DRRT_Q.jl:3249).  parent_edge[v] (may be NULL) = the id of the mirrored edge v -> rrtParent(v): the lowest id
 * among the edges that attain the minimum (-1: the root, or an orphan).  passes (may be NULL) = relaxation
 * passes run.  CONTRACT: changeThresh = 0 run to exhaustion only -- a positive changeThresh (the value the one
 * runnable script passes, R/experimentsForRRTQX.jl:30,132) and the goal-bounded loop of reduceInconsistency
 * (R/DRRT_Q.jl:2706) make the reference's result depend on its pop order; that epsilon-consistent variant is not
 * offered and stays on the host.  A solve that cannot reach a fixed point (a pass limit, a parent structure that is
 * no forest, a HIP error part-way) returns RRTX_E_STATE / RRTX_E_DEVICE and FORGETS the previous solve: the next
 * rrtx_graph_cost_update then solves in full.
 * rrtx_graph_cost_update gives the same answer starting from the state the previous call (either function, same
 * root) left on the device: nodes and edges appended since then, costs changed with set_dist / block.  This is
 * the replanning step: edges whose cost was touched and that were parent edges orphan their subtrees
 * (propogateDescendants, R/DRRT_Q.jl:2760-2817), orphans restart at Inf, and only the region that changes is
 * relaxed again.  Without a previous solve for this root it is rrtx_graph_cost_to_root.
 * The mirror also keeps edge.distOriginal: the SimpleEdge cost written by rrtx_graph_edges_append, replaced by every
 * value rrtx_graph_edges_set_dist writes -- Inf included: a caller that blocks through set_dist has replaced the
 * original.  rrtx_graph_edges_block and the `block` of rrtx_obstacle_sweep_batch leave it alone.
 * rrtx_graph_edges_unblock is the counterpart of rrtx_graph_edges_block, removeObstacle's `edge.dist =
 * edge.distOriginal` (R/DRRT_Q.jl:3342): dist = distOriginal for every id, marked as touched for the next
 * rrtx_graph_cost_update.  An id outside the mirror is RRTX_E_INVALID and nothing is written; an id that is not
 * blocked is rewritten with its own value; n == 0 is RRTX_OK. */
int rrtx_graph_edges_set_dist(rrtx_ctx *ctx, int64_t first_id, const double *dist, int64_t n);
int rrtx_graph_edges_block(rrtx_ctx *ctx, const int32_t *edge_ids, int64_t n);
int rrtx_graph_edges_unblock(rrtx_ctx *ctx, const int32_t *edge_ids, int64_t n);
int rrtx_graph_cost_to_root(rrtx_ctx *ctx, int root_idx, double *lmc /* n_nodes */, int32_t *parent_edge /* n_nodes */,
                            int32_t *passes);
int rrtx_graph_cost_update(rrtx_ctx *ctx, int root_idx, double *lmc /* n_nodes */, int32_t *parent_edge /* n_nodes */,
                           int32_t *passes);
/* rrtx_graph_cost_update that reports the nodes it changed instead of every node: what propogateDescendants /
 * reduceInconsistency (R/DRRT_Q.jl:2647-2817) hand their caller -- the new orphans, the nodes whose rrtLMC moved, the
 * nodes with another parent edge.  The solve is exactly that of rrtx_graph_cost_update(ctx, root_idx, ...): the same
 * resume rule, fixed point, parent rule (lowest edge id that attains the minimum) and failure behaviour (a failing
 * solve forgets the previous solve); it leaves the solver state rrtx_graph_cost_update would leave, so the two calls
 * mix freely.
 *   Baseline: the context remembers what this call last reported -- a root and, per node, the 64-bit pattern of its
 *     rrtLMC and its parent edge.  A node beyond the remembered count, or every node when the remembered root is not
 *     root_idx, counts as reported +Inf / -1 (rrtx_node_cost_set's convention for a node never set).
 *   Output: the nodes v whose rrtLMC (compared as a bit pattern) or parent edge differs from the baseline, ascending:
 *     node[i] = v, lmc[i] = its rrtLMC (+Inf: an orphan), parent_edge[i] = its parent edge id (-1: the root or an
 *     orphan; parent_edge may be NULL, changes are judged on both fields all the same).  The first call for a root
 *     returns every node that reaches the root and the root itself (lmc 0 against +Inf); a call after which nothing
 *     differs returns *needed = 0.
 *   Capacity, two-call pattern: more than cap changed nodes is RRTX_E_CAPACITY with *needed set, the baseline NOT
 *     advanced and the three arrays unspecified; the next call with room returns the same list (its solve has nothing
 *     new to do).  cap == 0 with NULL arrays counts only.  RRTX_OK advances the baseline to the solver's state of all
 *     n_nodes nodes.
 *   store != 0: whenever the solve itself succeeded (RRTX_OK or RRTX_E_CAPACITY) the context's own rrtLMC array --
 *     the one rrtx_node_cost_set writes and lmc == NULL reads in rrtx_extend_select / rrtx_find_new_target -- holds the
 *     solver's value of every node 0 .. n_nodes-1, copied on the device bit for bit over whatever was there.
 *     store == 0 leaves that array alone.
 *   Errors: RRTX_E_INVALID for cap < 0, cap > 0 with node or lmc NULL, needed NULL, a root outside the tree; what
 *     rrtx_graph_cost_update refuses is refused alike (RRTX_E_STATE on an empty tree).  A failing call keeps the
 *     baseline: what the caller was told still stands.  rrtx_graph_edges_clear forgets the baseline (the remembered
 *     edge ids die with the mirror). */
int rrtx_graph_cost_update_delta(rrtx_ctx *ctx, int root_idx, int store, int32_t *node, double *lmc, int32_t *parent_edge,
                                 int64_t cap, int64_t *needed, int32_t *passes);
/* cullCurrentNeighbors over the mirror (R/DRRT_Q.jl:2388-2403), and the removal of what it dropped.
 * RRT^X bounds every node's degree: whenever a node is rewired or has its rrtLMC recalculated it drops its CURRENT
 * out-neighbours whose edge.dist exceeds the ball, which shrinks as the tree grows, and keeps its INITIAL ones.
 * Node indices are insertion order and extend() alone makes edges -- new -> neighbour is the new node's initial
 * out-neighbour, neighbour -> new the older node's current one -- so A MIRRORED EDGE IS A CURRENT OUT-EDGE OF ITS START
 * NODE IFF start < end.  That holds for what rrtx_graph_edges_append_selected / _append_lists[_dev] produce (tree lists,
 * self lists, the closestNode rule) and classifies what rrtx_graph_edges_append registers the same way; a self loop is
 * never current.
 * rrtx_graph_edges_cull: cullCurrentNeighbors(node, ball) for the k nodes listed (a node listed twice is fine), or
 * for every node when nodes is NULL and k is 0.  Every mirrored edge that is not yet culled, whose start node is
 * listed, with start < end and dist > ball becomes CULLED.  The comparison is IEEE on the edge.dist the mirror holds
 * (whatever wrote it, in any dimension): a NaN cost is kept, dist == ball is kept, a blocked edge (+Inf) is culled.
 * A culled edge gets dist = distOriginal = +Inf, is marked as touched for the next rrtx_graph_cost_update exactly as
 * rrtx_graph_edges_block marks it, and carries a culled flag of its own.  To every other call it is an edge blocked for
 * good: the next rrtx_graph_cost_update[_delta] orphans the nodes whose parent edge it was and solves again;
 * rrtx_graph_edges_unblock and the `unblock` of the release calls restore +Inf; until the mirror is compacted the
 * sweeps and releases may still list its id.  Writing a finite cost to a culled id with rrtx_graph_edges_set_dist
 * does not clear the flag: the edge relaxes again, and rrtx_graph_edges_compact refuses (RRTX_E_STATE) for as long as
 * a solve uses it as a parent edge.  *n_culled (may be NULL) = the edges this call culled; the same call again culls
 * 0.  ball NaN or negative, k < 0, k > 0 with nodes NULL, a node outside the tree: RRTX_E_INVALID, nothing written.  An
 * empty mirror, or k == 0 with nodes given: RRTX_OK and 0.
 * WHAT THIS IS NOT: inside the reference's queue loop a finite ball depends on pop order -- a node can be improved
 * through a long edge before it is itself popped and culled.  The device offers the order-independent object, the
 * fixed point over the culled graph (cull, then rrtx_graph_cost_update), and does not claim equality with
 * reduceInconsistency run with a finite hyberBallRad.
 * rrtx_graph_edges_compact removes the culled edges.  Survivors keep their order: new id = old id - (culled edges
 * with a lower id); start, end, dist, distOriginal and a pending touched mark move together, no survivor is culled,
 * rrtx_graph_edges_count shrinks and the next append starts there.  remap (may be NULL; else remap_cap >= the edge count
 * at entry, RRTX_E_CAPACITY with nothing changed otherwise) receives remap[old] = new, -1 for a removed edge.  The
 * kept solver state is carried over: the parent edges are renumbered on the device, so is the baseline of
 * rrtx_graph_cost_update_delta -- a baseline entry whose edge was removed becomes a value no id equals, and that node
 * is reported by the next delta -- and the next solve rebuilds its in-edge index.  PRECONDITION, decided on the
 * device: when a kept solve still has a culled edge as some node's parent edge (compaction straight after a cull; a
 * culled id revived with set_dist) the call is RRTX_E_STATE -- run rrtx_graph_cost_update first -- and nothing
 * changes.  Without a kept solve it always goes through.  *n_removed (may be NULL) = edges removed.
 * rrtx_graph_edges_get_culled: culled[i] = 1 when edge first_id + i is culled, else 0 (rrtx_graph_edges_get cannot
 * tell a cull from set_dist(+Inf)); a range outside the mirror is RRTX_E_INVALID.  rrtx_graph_edges_clear clears the
 * flags with the mirror.  The three calls keep the lists of rrtx_extend_select (HOLD RULE below). */
int rrtx_graph_edges_cull(rrtx_ctx *ctx, double ball, const int32_t *nodes, int64_t k, int64_t *n_culled);
int rrtx_graph_edges_compact(rrtx_ctx *ctx, int32_t *remap, int64_t remap_cap, int64_t *n_removed);
int rrtx_graph_edges_get_culled(rrtx_ctx *ctx, int64_t first_id, int64_t n, uint8_t *culled);
/* explicitPointCheck (R/DRRT_Q.jl:1520-1556; quick=0: explicitPointCheck3D,
 * :1558-1590).  unsafe[i] in {0,1}; clearance[i] = the returned certificate
 * (0.0 when unsafe); clearance may be NULL when only the flag is wanted (the
 * same obstacles are looked at either way). kind as above. */
int rrtx_points_check(rrtx_ctx *ctx, int kind, const double *p, int64_t np, double robot_radius,
                      int quick, uint8_t *unsafe, double *clearance);

/* ---- steering (A6, A7, A11) -------------------------------------------------- */
/* calculateTrajectory(S, ::SimpleEdge) (R/DRRT_SimpleEdge_functions.jl:177-181):
 * dist over all dim coordinates, wdist over the first 3. */
int rrtx_simple_steer(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double *dist,
                      double *wdist);
/* calculateTrajectory(S, ::DubinsEdge) (R/DRRT_DubinsEdge_functions.jl:329-501),
 * space without time: cost = edge.dist = edge.Wdist, word = 3 chars per edge
 * ("rsl","rsr","rlr","lsr","lsl","lrl","xxx").  s, g are ne x 4 [x y t theta]. */
int rrtx_dubins_steer(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                      double *cost, uint8_t *word /* ne x 3 */);
/* S.dubinsMinVelocity / S.dubinsMaxVelocity (R/DRRT_data_structures.jl:354-355), read by validMove in a space
 * with time.  Default: no bounds. */
int rrtx_set_dubins_velocity(rrtx_ctx *ctx, double v_min, double v_max);
/* calculateTrajectory's scalar results in full: dist = edge.dist (== Wdist without time, sqrt(Wdist^2 + dt^2)
 * with), wdist = edge.Wdist, velocity = edge.velocity (0 without time), valid_move = validMove(S, edge)
 * (always 1 without time).  Any output may be NULL. */
int rrtx_dubins_steer_full(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min, double *dist,
                           double *wdist, double *velocity, uint8_t *word /* ne x 3 */, uint8_t *valid_move);
/* Same, plus the discretised trajectory (:506-701) and the two-stage Dubins
 * collision check against the polygon list (:750-774).  traj_len[i] = number of
 * polyline rows the reference builds (may be NULL). */
int rrtx_dubins_edges_check(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne,
                            double r_min, double robot_radius, double *cost, uint8_t *word,
                            uint8_t *hit, int32_t *traj_len);

/* explicitEdgeCheck(S, edge::DubinsEdge, ob) (:750-774) against ONE obstacle of the polygon list (list position;
 * an obstacle not in use collides with nothing, R/DRRT.jl:1525): what addNewObstacle asks per edge (R/DRRT.jl:3157). */
int rrtx_dubins_edges_check_obstacle(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                                     double robot_radius, int obstacle, uint8_t *hit);

/* edge.trajectory of calculateTrajectory(S, ::DubinsEdge) (:506-701): the discretised polyline
 * (0.1 rad arc steps, Julia float-range length rule), P_i rows of (x, y) per edge -- rows of (x, y, t) with
 * RRTX_OPT_SPACE_HAS_TIME, the last row being the end node's (x, y, t) (:684-696) -- CSR layout:
 * traj_off[ne+1] (rows), traj_xy[cols * total rows].  `cols` is the row width the caller's buffer was sized
 * for and must be the context's (2, or 3 with RRTX_OPT_SPACE_HAS_TIME; rrtx_get_option tells): anything else is
 * RRTX_E_INVALID and nothing is written -- a caller whose idea of the space drifted from the context's gets an
 * error, not a buffer overrun.  Two-call pattern: if the total exceeds cap_rows the call returns
 * RRTX_E_CAPACITY with *needed_rows set (traj_off is still valid). */
int rrtx_dubins_trajectory(rrtx_ctx *ctx, const double *s, const double *g, int64_t ne, double r_min,
                           int64_t *traj_off, double *traj_xy, int cols, int64_t cap_rows, int64_t *needed_rows);

/* Diagnostics: the deterministic transcendentals of include/rrtx_detmath.h evaluated ON THE DEVICE, element-wise
 * over host arrays (op 0 sin(x), 1 cos(x), 2 atan2(y, x), 3 acos(x); y may be NULL for the one-argument ops).
 * The parity suite holds the device build of that header against the host build bit for bit with it. */
int rrtx_detmath_eval(rrtx_ctx *ctx, int op, const double *x, const double *y, int64_t n, double *out);

/* ---- fused per-sample preamble of extend() (A13) ----------------------------- */
/* For each of nq samples: kdFindWithinRange + for every neighbour both directed
 * SimpleEdges sample->near and near->sample: calculateTrajectory cost and
 * explicitEdgeCheck over the sphere list (R/DRRT_Q.jl:1927-1979, 2581-2637),
 * plus kdFindNearest (R/rrtqx.jl:926) and explicitPointCheck of the sample
 * (R/rrtqx.jl:940).  CSR layout as rrtx_nn_radius; per neighbour entry:
 * cost (same both ways for SimpleEdge), hit_out (sample->near), hit_in. */
int rrtx_extend_candidates(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                           int64_t *offsets, int32_t *idx, double *cost, uint8_t *hit_out,
                           uint8_t *hit_in, int64_t cap, int64_t *needed, int32_t *nearest_idx,
                           double *nearest_dist, uint8_t *sample_unsafe);

/* ---- the samples of one extend batch among themselves ------------------------- */
/* The lists of rrtx_extend_candidates are against the tree as it stood: the samples of one batch do not see each
 * other there.  This call supplies the rest.  For a batch q of nq samples it gives, per sample j, the samples i < j of
 * the same batch with KDdist(q_j, q_i) < r -- exactly what kdFindWithinRange (R/kdTree_general.jl:830) adds to j's
 * list when the samples are inserted one after the other -- with the SimpleEdge cost and both collision flags of
 * extend (R/DRRT_Q.jl:1927-1979, 2581-2637).  The tree list of rrtx_extend_candidates followed by this list, with
 * idx mapped to the node index each earlier sample received (entries of samples that were not inserted dropped), is
 * the reference's list; the order stays ascending because the mapping is monotone.
 *   Scope    SimpleEdge only: dim == 3 and no wrapped dimension, otherwise RRTX_E_STATE as in rrtx_extend_candidates;
 *            bad pointers or negative counts are RRTX_E_INVALID; a radius is taken as rrtx_extend_candidates takes it
 *            (r <= 0 or NaN: every list is empty).  Obstacles: the spheres or the polygons by
 *            RRTX_OPT_EXTEND_OBSTACLES; kinds 6 / 7 read time from the third coordinate.  The tree is not read: the
 *            call works whatever the tree holds, an empty tree included.  The Dubins lists come from
 *            rrtx_extend_candidates_self_dubins; a radius per sample is out of scope.
 *   Lists    CSR offsets[nq + 1] from 0.  Row j: the batch positions i < j, ascending, with s = sq3(q_j, q_i) < thr,
 *            thr = the first_ge threshold of r (rrtx_sq_thresholds), the test the range search applies to a non-root
 *            node.  There is no root rule: the root is a tree node, never a sample.  idx[e] = i, a 0-based position
 *            in q, not a node index.
 *   Entries  cost[e] = sqrt(s), correctly rounded: the key and the SimpleEdge cost at once.  hit_out[e] =
 *            explicitEdgeCheck of the directed edge q_j -> q_i (new node -> earlier node), hit_in[e] of q_i -> q_j,
 *            both by the kernels of rrtx_extend_candidates -- a zero-length edge collides with every active sphere
 *            (two equal samples are neighbours at cost 0).  inWarmupTime stays with the caller.
 *   skip     nq bytes or NULL.  A sample with skip[j] != 0 has an empty list and appears in no list; the
 *            sample_unsafe bytes of the rrtx_extend_candidates call on the same batch can be passed as they are.
 *            A sample with a non-finite coordinate likewise has an empty list and appears in none (no comparison with
 *            NaN / Inf is true) and does not disturb the lists of the others.
 *   Capacity the two-call pattern of rrtx_extend_candidates: more than cap entries is RRTX_E_CAPACITY with *needed set
 *            and offsets valid; cap == 0 (arrays may be NULL) counts; nq == 0 is RRTX_OK with offsets[0] = 0.
 * Exact, no tolerance; nothing in the result depends on launch geometry or on the order in which waves finish. */
int rrtx_extend_candidates_self(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                const uint8_t *skip, int64_t *offsets, int32_t *idx, double *cost,
                                uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed);

/* ---- the closestNode rule for an extend batch: k nearest earlier samples -------- */
/* A sample whose ball is empty is linked to closestNode (findBestParent, R/DRRT_Q.jl:1930-1935), which is kdFindNearest
 * over the tree as sequential insertion would have it: it may be an earlier sample of the same batch.
 * rrtx_extend_candidates gives the nearest node of the tree as it stood, rrtx_extend_candidates_self only the earlier
 * samples inside the ball, and the long edge to closestNode is not served by their per-sample obstacle lists.  This call
 * supplies the rest: per wanted sample j a short sorted row of its nearest live earlier samples, each with the SimpleEdge
 * cost and both collision flags against the whole obstacle list, and the same flags for one tree node per sample.
 * Whether an earlier sample was inserted is decided by the caller's sequential phase, which the device cannot know;
 * hence a row of k instead of one index.
 *   Scope    SimpleEdge only: dim == 3 and no wrapped dimension, otherwise RRTX_E_STATE as in
 *            rrtx_extend_candidates_self.  1 <= k <= RRTX_CLOSEST_SELF_MAX_K, nq >= 0, non-NULL outputs when nq > 0,
 *            tree_idx / tree_hit_out / tree_hit_in all NULL or all given; otherwise RRTX_E_INVALID.  Obstacles: the
 *            spheres or the polygons by RRTX_OPT_EXTEND_OBSTACLES; kinds 6 / 7 read time from the third coordinate.
 *            Apart from tree_idx the tree is not read; an empty tree is fine.  The Dubins spaces ([x y t theta], wrapped
 *            dimensions, rrtx_extend_candidates_self_dubins) are out of scope here: rrtx_extend_closest_self_dubins.
 *   Live     a sample is live when every coordinate is finite and skip[j] == 0 (skip: nq bytes or NULL; the
 *            sample_unsafe bytes of rrtx_extend_candidates can be passed as they are).
 *   Rows     idx, cost, hit_out, hit_in are nq x k, row-major, as in rrtx_nn_knearest; count is nq.  Row j is filled iff
 *            j is live and (want == NULL or want[j] != 0).  A filled row holds the live samples i < j with finite
 *            s = sq3(q_j, q_i) (the unfused fp64 expression of rrtx_extend_candidates_self), ordered by (s, i)
 *            ascending: the first min(k, their number) of them, count[j] says how many.  Unused slots and rows that are
 *            not filled have idx = -1, cost = +Inf, flags 0, count = 0.  idx is a 0-based position in q, not a node
 *            index.  A sample with want[j] == 0 is still a candidate in the rows of the others: the caller sets want
 *            where the tree list of rrtx_extend_candidates is empty, and with no row wanted the call costs a few launches.
 *   Entries  cost = sqrt(s), correctly rounded: the key and the SimpleEdge cost at once.  hit_out = explicitEdgeCheck of
 *            q_j -> q_i, hit_in of q_i -> q_j, over the WHOLE active obstacle list: byte for byte what rrtx_edges_check
 *            returns for that directed edge.
 *   Tree     for a filled row with 0 <= tree_idx[j] < rrtx_nodes_count, tree_hit_out[j] / tree_hit_in[j] are the same
 *            full-list flags of q_j -> node and node -> q_j; otherwise 0 (an index out of range is not an error).  With
 *            nearest_idx of rrtx_extend_candidates as tree_idx the one call hands the caller all the rule needs.
 *   The rule walk row j and take the first entry whose sample was inserted.  Link to it if its cost < nearest_dist[j],
 *            else to nearest_idx[j] (on an exact tie the tree node, which has the lower index, wins, as in
 *            rrtx_nn_nearest).  If count[j] == k and none of the k was inserted the row is exhausted: the caller then
 *            finds the nearest inserted earlier sample itself (brute force over the batch, then two rrtx_edges_check
 *            calls).  It need not when the k-th cost is not below nearest_dist[j]: no later entry beats the tree node.
 * Exact, no tolerance; nothing in the result depends on launch geometry or on the order in which waves finish. */
#define RRTX_CLOSEST_SELF_MAX_K 32
int rrtx_extend_closest_self(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius,
                             const uint8_t *skip, const uint8_t *want, const int32_t *tree_idx,
                             int32_t *idx, double *cost, uint8_t *hit_out, uint8_t *hit_in, int32_t *count,
                             uint8_t *tree_hit_out, uint8_t *tree_hit_in);

/* The same preamble for Edge = DubinsEdge (BASELINE config 3; R/dubinsExperimentsForPaper.jl): tree in
 * [x y t theta] with theta wrapped (rrtx_set_wrap), polygon obstacle list.  Per neighbour entry:
 * key = the KDdist the range search stores, Dubins cost and word for sample->near (out) and
 * near->sample (in), and the two-stage Dubins collision flags (R/DRRT_DubinsEdge_functions.jl:750-774).
 * With RRTX_OPT_SPACE_HAS_TIME the costs are edge.dist in [x y t theta] and a flag byte also carries
 * bit 1 (value 2) = !validMove(S, edge): findBestParent blocks an edge on either (R/DRRT_Q.jl:1960), so the
 * caller's test is simply hit != 0.
 * word_out / word_in (3 bytes per entry) and nearest_* / sample_unsafe may be NULL. */
int rrtx_extend_candidates_dubins(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                  double r_min, int64_t *offsets, int32_t *idx, double *key, double *cost_out,
                                  double *cost_in, uint8_t *word_out, uint8_t *word_in, uint8_t *hit_out,
                                  uint8_t *hit_in, int64_t cap, int64_t *needed, int32_t *nearest_idx,
                                  double *nearest_dist, uint8_t *sample_unsafe);

/* ---- the samples of one Dubins extend batch among themselves ------------------- */
/* What rrtx_extend_candidates_self is to rrtx_extend_candidates, for Edge = DubinsEdge: the lists of
 * rrtx_extend_candidates_dubins are against the tree as it stood, this call gives, per sample j of a batch q
 * (nq x 4, [x y t theta]), the batch positions i < j that kdFindWithinRange (R/kdTree_general.jl:830) and its ghost
 * iterator (R/ghostPoint.jl:60-111) add to j's list when the samples are inserted one after the other.  The tree list
 * of rrtx_extend_candidates_dubins followed by this list, with idx mapped to the node index each earlier sample
 * received (entries of samples that were not inserted dropped), is the reference's list, keys included.
 *   Scope    dim == 4, otherwise RRTX_E_STATE; the wrapped dimensions are the context's (rrtx_set_wrap, 0 to 3 of them);
 *            bad pointers or negative counts are RRTX_E_INVALID; r <= 0 or NaN: every list is empty.  The tree is not
 *            read.  A radius per sample is out of scope.
 *   Copies   the query is sample j with its 2^w copies, by the rule of the range search: slot 0 is the sample, slot k
 *            shifts the wrapped dimensions whose bit is set in k (the last wrapped dimension is the least significant
 *            bit); a shifted coordinate p < period / 2 becomes p + period with closest unwrapped coordinate period,
 *            otherwise p - period with closest unwrapped coordinate 0; a ghost is skipped when
 *            sq4(closest, ghost) >= the first_gt threshold of r.  The earlier sample i is taken as it is.
 *   Lists    CSR offsets[nq + 1] from 0.  Entry (j, i) exists iff both samples are live, i < j and some non-skipped
 *            slot k has s_k = sq4(copy_k(q_j), q_i) < thr, thr = the first_ge threshold of r (rrtx_sq_thresholds).
 *            key[e] = sqrt(s_k), correctly rounded, of the LOWEST such k: addToRangeList keeps the first discovery.
 *            There is no root rule.  Rows are ascending in i; idx[e] = i is a 0-based position in q.
 *   Entries  cost_out / word_out / hit_out: the directed Dubins edge q_j -> q_i (new node -> earlier node);
 *            cost_in / word_in / hit_in: q_i -> q_j; by the steering and check kernels of
 *            rrtx_extend_candidates_dubins, so RRTX_OPT_SPACE_HAS_TIME (bit 1 of a flag byte = !validMove),
 *            rrtx_set_dubins_velocity, RRTX_OPT_DUBINS_TIME_COLUMN, moving polygons and the active flags hold as
 *            there.  word_out / word_in (3 bytes per entry) may be NULL.
 *   skip     nq bytes or NULL.  A sample with skip[j] != 0 has an empty list and appears in no list; the
 *            sample_unsafe bytes of the rrtx_extend_candidates_dubins call on the same batch can be passed as they
 *            are.  A sample with a non-finite coordinate, in any of the four, likewise.
 *   Capacity the two-call pattern: more than cap entries is RRTX_E_CAPACITY with *needed set and offsets valid;
 *            cap == 0 (arrays may be NULL) counts; nq == 0 is RRTX_OK with offsets[0] = 0.
 * Exact, no tolerance; nothing in the result depends on launch geometry or on the order in which waves finish. */
int rrtx_extend_candidates_self_dubins(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                       double r_min, const uint8_t *skip, int64_t *offsets, int32_t *idx, double *key,
                                       double *cost_out, double *cost_in, uint8_t *word_out, uint8_t *word_in,
                                       uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed);

/* ---- the closestNode rule for a Dubins extend batch: k nearest in wrapped space - */
/* What rrtx_extend_closest_self is to the SimpleEdge spaces, for Edge = DubinsEdge: a sample whose ball is empty is linked
 * to closestNode (findBestParent, R/DRRT_Q.jl:1930-1935), kdFindNearest over the tree as sequential insertion would have
 * it, which may be an earlier sample of the same batch.  Per wanted sample j of a batch q (nq x 4, [x y t theta]) this
 * call gives its k nearest live earlier samples in the context's wrapped space, per entry what
 * rrtx_extend_candidates_dubins reports (key, both Dubins costs, both words, both flag bytes), and the same for one tree
 * node per sample.
 *   Scope    dim == 4, otherwise RRTX_E_STATE; the wrapped dimensions are the context's (rrtx_set_wrap, 0 to 3 of them).
 *            1 <= k <= RRTX_CLOSEST_SELF_MAX_K, nq >= 0, non-NULL outputs when nq > 0 except word_out, word_in,
 *            tree_word_out, tree_word_in, which may be NULL; tree_idx, tree_cost_out, tree_cost_in, tree_hit_out,
 *            tree_hit_in all NULL or all given (the tree words are not written without them); anything else is
 *            RRTX_E_INVALID.  Obstacles: the polygon list, as in rrtx_extend_candidates_dubins.  Apart from tree_idx the
 *            tree is not read; an empty tree is fine.
 *   Live     a sample is live when all four coordinates are finite and skip[j] == 0 (skip: nq bytes or NULL).
 *   Copies   sample j has 2^w copies by the rule of rrtx_extend_candidates_self_dubins, in its slot order: a shifted
 *            coordinate p < period / 2 becomes p + period, anything else p - period.  NO copy is skipped: there is no
 *            radius to skip by.  The column sample i is taken as it is.
 *   Rows     idx, key, cost_out, cost_in, hit_out, hit_in are nq x k, row-major, word_out / word_in nq x k x 3 bytes;
 *            count is nq.  s(j, i) = min over all 2^w slots of sq4(copy_slot(q_j), q_i), sq4 the unfused left-to-right
 *            fp64 expression.  Row j is filled iff j is live and (want == NULL or want[j] != 0).  A filled row holds the
 *            live i < j with finite s, ordered by (s, i) ascending: the first min(k, their number) of them, count[j]
 *            says how many.  key = sqrt(s), correctly rounded.  Unused slots and rows that are not filled have idx = -1,
 *            key = cost_out = cost_in = +Inf, words three zero bytes, flags 0, count = 0.  idx is a 0-based position in
 *            q.  want only chooses rows: a sample with want[j] == 0 is still a candidate in the rows of the others.
 *   Entries  cost_out / word_out / hit_out: the directed Dubins edge q_j -> q_i; cost_in / word_in / hit_in: q_i -> q_j;
 *            by the steering and check kernels of rrtx_extend_candidates_dubins over the WHOLE polygon list, so
 *            RRTX_OPT_SPACE_HAS_TIME (bit 1 of a flag byte = !validMove), rrtx_set_dubins_velocity,
 *            RRTX_OPT_DUBINS_TIME_COLUMN, moving polygons and the active flags hold as there: byte for byte and bit for
 *            bit what rrtx_dubins_edges_check (plus validMove with time) returns for that edge.
 *   Tree     a filled row with 0 <= tree_idx[j] < rrtx_nodes_count gets the same fields for q_j <-> node in tree_cost_out
 *            / tree_word_out / tree_hit_out (q_j -> node) and tree_cost_in / tree_word_in / tree_hit_in; otherwise cost
 *            +Inf, words and flags 0 (an index out of range is not an error).  nearest_idx of
 *            rrtx_extend_candidates_dubins is the intended input.
 *   The rule as for rrtx_extend_closest_self: walk row j and take the first entry whose sample was inserted.  Link to it
 *            if key < nearest_dist[j], else to the tree node (on a tie the tree node, which has the lower index, wins).
 *            A row with count[j] == k and no inserted entry is exhausted: the caller then searches the batch itself and
 *            calls rrtx_dubins_edges_check twice.  It need not when the k-th key is not below nearest_dist[j].
 *   kdFindNearest  the reference hands out a ghost only while dist(closest unwrapped point, ghost) is not above the best
 *            distance so far.  For a column whose wrapped coordinates lie in [0, period] every term of
 *            sq4(ghost, column) is at least the matching term of sq4(closest, ghost) and fp rounding is monotone, so a
 *            skipped ghost never improves the minimum and the row's order is kdFindNearest's.  The guarantee holds for
 *            samples inside the period in their wrapped coordinates, which is what the planner draws; outside the period
 *            the row is still exactly as defined above.
 * Exact, no tolerance; nothing in the result depends on launch geometry or on the order in which waves finish. */
int rrtx_extend_closest_self_dubins(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius, double r_min,
                                    const uint8_t *skip, const uint8_t *want, const int32_t *tree_idx, int32_t *idx,
                                    double *key, double *cost_out, double *cost_in, uint8_t *word_out, uint8_t *word_in,
                                    uint8_t *hit_out, uint8_t *hit_in, int32_t *count, double *tree_cost_out,
                                    double *tree_cost_in, uint8_t *tree_word_out, uint8_t *tree_word_in,
                                    uint8_t *tree_hit_out, uint8_t *tree_hit_in);

/* ---- device-resident variants (inputs/outputs are DEVICE pointers) ------------ */
int rrtx_nn_nearest_dev(rrtx_ctx *ctx, const double *q, int nq, int32_t *idx, double *dist);
/* rows max(k, 2) wide as in rrtx_nn_knearest.  The list path (RRTX_OPT_KNN_LISTS) reads two small values
 * back from the device on the way (its radius guess and the size of the lists), so this call waits on the
 * stream internally; the result kernels themselves are only enqueued. */
int rrtx_nn_knearest_dev(rrtx_ctx *ctx, const double *q, int nq, int k, int32_t *idx, double *dist, int32_t *count);
int rrtx_nn_radius_dev(rrtx_ctx *ctx, const double *q, double r, int nq, int64_t *offsets,
                       int32_t *idx, double *dist, int64_t cap, int64_t *needed_dev);
int rrtx_edges_check_dev(rrtx_ctx *ctx, int kind, const double *p0, const double *p1, int64_t ne,
                         double robot_radius, int obstacle_or_minus1, int obs_begin, int obs_end,
                         uint8_t *hit, int32_t *first_hit);
int rrtx_points_check_dev(rrtx_ctx *ctx, int kind, const double *p, int64_t np, double robot_radius,
                          int quick, uint8_t *unsafe, double *clearance);
int rrtx_extend_candidates_dev(rrtx_ctx *ctx, const double *q, int nq, double r,
                               double robot_radius, int64_t *offsets, int32_t *idx, double *cost,
                               uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed_dev,
                               int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe);

/* device-pointer form of rrtx_extend_candidates_self (skip may be NULL): *needed_dev receives the number of entries, no
 * entry at or beyond cap is written (with more than cap entries none is, offsets stays valid).  Only enqueues; the
 * growth of a workspace may wait on the stream once. */
int rrtx_extend_candidates_self_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                    const uint8_t *skip, int64_t *offsets, int32_t *idx, double *cost,
                                    uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed_dev);

/* device-pointer form of rrtx_extend_closest_self (skip, want and the three tree arrays may be NULL as there).  Only
 * enqueues, never waits on the stream (the growth of a workspace may, once); every read of q and tree_idx and every
 * write is bounded by nq, k and the node count on the device. */
int rrtx_extend_closest_self_dev(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius,
                                 const uint8_t *skip, const uint8_t *want, const int32_t *tree_idx,
                                 int32_t *idx, double *cost, uint8_t *hit_out, uint8_t *hit_in, int32_t *count,
                                 uint8_t *tree_hit_out, uint8_t *tree_hit_in);

/* device-pointer form of rrtx_extend_candidates_dubins; *needed_dev receives the number of entries (entries
 * beyond cap are not written).  Only enqueues work, never waits on the stream: with wrapped dimensions nearest_*
 * come from the nearest scan (rrtx_nn_nearest_dev: records a full candidate buffer dropped are re-decided by its
 * fix-up pass on the device); without them they come off the lists, and a sample whose ball is empty gets
 * kdFindNearest's answer from the expanding search of the finish kernel -- no -1 leaves the device. */
int rrtx_extend_candidates_dubins_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                      double r_min, int64_t *offsets, int32_t *idx, double *key, double *cost_out,
                                      double *cost_in, uint8_t *word_out, uint8_t *word_in, uint8_t *hit_out,
                                      uint8_t *hit_in, int64_t cap, int64_t *needed_dev, int32_t *nearest_idx,
                                      double *nearest_dist, uint8_t *sample_unsafe);

/* device-pointer form of rrtx_extend_candidates_self_dubins (skip, word_out, word_in may be NULL): *needed_dev receives
 * the number of entries, no entry at or beyond cap is written (with more than cap entries none is, offsets stays
 * valid).  Only enqueues; the growth of a workspace may wait on the stream once. */
int rrtx_extend_candidates_self_dubins_dev(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius,
                                           double r_min, const uint8_t *skip, int64_t *offsets, int32_t *idx,
                                           double *key, double *cost_out, double *cost_in, uint8_t *word_out,
                                           uint8_t *word_in, uint8_t *hit_out, uint8_t *hit_in, int64_t cap,
                                           int64_t *needed_dev);

/* device-pointer form of rrtx_extend_closest_self_dubins (skip, want, the four word arrays and the tree arrays may be NULL
 * as there).  Only enqueues; the growth of a workspace may wait on the stream once.  Every read of q and tree_idx and
 * every write is bounded by nq, k and the node count on the device. */
int rrtx_extend_closest_self_dubins_dev(rrtx_ctx *ctx, const double *q, int nq, int k, double robot_radius, double r_min,
                                        const uint8_t *skip, const uint8_t *want, const int32_t *tree_idx, int32_t *idx,
                                        double *key, double *cost_out, double *cost_in, uint8_t *word_out,
                                        uint8_t *word_in, uint8_t *hit_out, uint8_t *hit_in, int32_t *count,
                                        double *tree_cost_out, double *tree_cost_in, uint8_t *tree_word_out,
                                        uint8_t *tree_word_in, uint8_t *tree_hit_out, uint8_t *tree_hit_in);

/* Per-edge collision bitmask for the multi-GPU exchange (RCCL all-reduce over
 * xGMI): bit e (e < cap) = hit_out[e], bit cap+e = hit_in[e]; entries at or
 * beyond *n_valid_dev read as 0.  words has (2*cap+63)/64 uint64 entries. */
/* device-pointer forms of rrtx_graph_cost_to_root / _update (they wait on the stream between groups of passes to learn whether
 * the fixed point is reached) */
int rrtx_graph_cost_to_root_dev(rrtx_ctx *ctx, int root_idx, double *lmc_dev, int32_t *parent_edge_dev);
int rrtx_graph_cost_update_dev(rrtx_ctx *ctx, int root_idx, double *lmc_dev, int32_t *parent_edge_dev);

int rrtx_pack_hits_dev(rrtx_ctx *ctx, const uint8_t *hit_out, const uint8_t *hit_in,
                       const int64_t *n_valid_dev, int64_t cap, uint64_t *words);

/* ---- parent and rewire selection over the extend lists ------------------------ */
/* findBestParent (R/DRRT_Q.jl:1927-1979) and the rewire test of extend (:2619-2634) for a whole batch, over the
 * CSR lists rrtx_extend_candidates* wrote and rrtLMC of every node (lmc: one double per node, at least
 * rrtx_nodes_count long).  Exact, no tolerance: every output is an input value, an index or one rounded fp64 addition.
 * Per sample s, over its entries e in list order (ascending node index):
 *   status[s]       RRTX_SEL_UNSAFE     sample_unsafe is given and sample_unsafe[s] != 0: nothing else is computed
 *                                       (the driver skips extend for such a sample, R/rrtqx.jl:940);
 *                   RRTX_SEL_EMPTY      the list has no entry (the closestNode rule, :1931-1935, stays with the caller);
 *                   RRTX_SEL_NO_PARENT  no entry was adopted;
 *                   RRTX_SEL_OK         otherwise;
 *                   RRTX_SEL_OVERFLOW   (every sample) the extend call produced more entries than its cap.
 *   parent          best = +Inf; for each entry with hit_out[e] == 0 (the Dubins-with-time byte also carries !validMove:
 *                   the test is "byte is zero"): cand = lmc[idx[e]] + cost_out[e]; adopted when best > cand.  A NaN or
 *                   +Inf candidate is never adopted (an orphan is never a parent); of exactly equal candidates the
 *                   lowest list position wins.  parent_idx[s] = idx of the winner, parent_entry[s] = its CSR
 *                   position, lmc_new[s] = best; -1, -1, +Inf unless status[s] is RRTX_SEL_OK.
 *   rewire          (RRTX_SEL_OK only) every entry with hit_in[e] == 0, idx[e] != parent_idx[s] and
 *                   lmc[idx[e]] > lmc_new[s] + cost_in[e], as (rw_node = idx[e], rw_value = lmc_new[s] + cost_in[e]) in
 *                   list order: a second CSR rw_offsets[nq + 1], rw_node, rw_value with the two-call capacity pattern.
 * For SimpleEdge lists pass the one cost array as cost_out and cost_in.  The kd-tree root needs no special case:
 * lmc[root] = 0 never exceeds a non-negative sum.  The lists are against the tree as it stood, as in
 * rrtx_extend_candidates (the samples' lists among themselves come from rrtx_extend_candidates_self), so a node may
 * appear in the rewire lists of several samples; settling that is the caller's bookkeeping. */
#define RRTX_SEL_OK 0
#define RRTX_SEL_NO_PARENT 1
#define RRTX_SEL_EMPTY 2
#define RRTX_SEL_UNSAFE 3
#define RRTX_SEL_OVERFLOW 4
/* Device-pointer form: only enqueues, never waits on the stream.  cap and n_valid_dev are the capacity the extend call
 * was given and the count it left on the device (needed_dev): with *n_valid_dev > cap every status is
 * RRTX_SEL_OVERFLOW and nothing else is written; no list entry at or beyond cap is read.  *rw_needed_dev receives the
 * number of rewire entries; entries at or beyond rw_cap are not written.  sample_unsafe may be NULL.  lmc == NULL
 * selects the context's own array (rrtx_node_cost_set), which may first have to grow with the nodes (that growth
 * waits on the stream once). */
int rrtx_extend_select_dev(rrtx_ctx *ctx, int nq, const int64_t *offsets, const int32_t *idx, const double *cost_out,
                           const double *cost_in, const uint8_t *hit_out, const uint8_t *hit_in,
                           const int64_t *n_valid_dev, int64_t cap, const uint8_t *sample_unsafe, const double *lmc,
                           int32_t *parent_idx, int64_t *parent_entry, double *lmc_new, uint8_t *status,
                           int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap,
                           int64_t *rw_needed_dev);
/* The context's own rrtLMC array on the device: one double per node, +Inf for a node never set, growing with
 * rrtx_nodes_append.  Writes lmc[0 .. n) to nodes first_index .. first_index + n - 1 (host pointer; the nodes must
 * exist), so a host planner uploads the few values a step changed instead of all of them. */
int rrtx_node_cost_set(rrtx_ctx *ctx, int64_t first_index, const double *lmc, int64_t n);
/* Host-pointer form for SimpleEdge (dim == 3, no wraps; spheres or polygons by RRTX_OPT_EXTEND_OBSTACLES): runs
 * rrtx_extend_candidates into buffers the context owns, then the selection, and returns the per-sample results and the
 * rewire lists only.  lmc: rrtLMC of every node (rrtx_nodes_count doubles), or NULL for the context's own array.
 * parent_entry is a position in the lists of THIS call (useful with the optional list outputs).  rw_* follow the two-call
 * pattern: with more than rw_cap rewire entries the call returns RRTX_E_CAPACITY with *rw_needed set (the per-sample
 * outputs and rw_offsets are valid).  nearest_idx / nearest_dist / sample_unsafe may be NULL (the samples are checked
 * either way: an unsafe sample has status RRTX_SEL_UNSAFE).  The neighbour lists themselves stay on the device unless
 * offsets is non-NULL: then offsets, idx, cost, hit_out, hit_in (room for cap entries, all non-NULL) and *needed receive
 * them as rrtx_extend_candidates would, RRTX_E_CAPACITY included. */
int rrtx_extend_select(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius, const double *lmc,
                       int32_t *parent_idx, int64_t *parent_entry, double *lmc_new, uint8_t *status,
                       int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap, int64_t *rw_needed,
                       int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe, int64_t *offsets,
                       int32_t *idx, double *cost, uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed);
/* Host-pointer form for DubinsEdge (dim == 4, [x y t theta]; RRTX_E_STATE otherwise).  Defined through existing calls:
 * rrtx_extend_candidates_dubins_dev on the staged samples into lists the context owns (word_out / word_in NULL), then
 * rrtx_extend_select_dev over them with cost_out and cost_in as TWO arrays (cost_out decides the parent, cost_in the
 * rewire test).  So it honours the wraps, RRTX_OPT_SPACE_HAS_TIME (a flag byte may then be 1, 2 or 3; the test stays
 * "byte is zero"), rrtx_set_dubins_velocity and RRTX_OPT_DUBINS_TIME_COLUMN, and reads the polygon list.  Everything
 * else is rrtx_extend_select's: lmc (NULL: the context's own array), the per-sample outputs, the rewire CSR with the
 * two-call pattern (RRTX_E_CAPACITY with *rw_needed set, the per-sample outputs and rw_offsets valid), nq == 0, the
 * growth of RRTX_OPT_SELECT_LIST_CAP with one more attempt.  The optional list outputs are offsets, idx, key, cost_out,
 * cost_in, hit_out, hit_in (all or none; offsets NULL: none), as rrtx_extend_candidates_dubins would write them.
 * nearest_idx / nearest_dist are kdFindNearest in the wrapped space (the minimum over the copies), which cannot be
 * read off the lists: the full nearest scan is enqueued after the range search, and writes only its own search
 * workspaces and the two per-sample columns.  Without wrapped dimensions the nearest is read off the lists and a
 * sample with an empty ball is resolved by the same scan inside this call.  Either way the lists this call leaves are
 * held (HOLD RULE below) whether or not the nearest was asked for; rrtx_extend_select drops them when its nearest
 * fallback has to search.  The held lists have three cost columns (key, cost_out, cost_in):
 * rrtx_graph_edges_append_selected links them with cost_out and cost_in. */
int rrtx_extend_select_dubins(rrtx_ctx *ctx, const double *q, int nq, double r, double robot_radius, double r_min,
                              const double *lmc, int32_t *parent_idx, int64_t *parent_entry, double *lmc_new,
                              uint8_t *status, int64_t *rw_offsets, int32_t *rw_node, double *rw_value, int64_t rw_cap,
                              int64_t *rw_needed, int32_t *nearest_idx, double *nearest_dist, uint8_t *sample_unsafe,
                              int64_t *offsets, int32_t *idx, double *key, double *cost_out, double *cost_in,
                              uint8_t *hit_out, uint8_t *hit_in, int64_t cap, int64_t *needed);

/* ---- the extend lists become mirror edges, on the device ------------------------ */
/* What extend() links for a batch (R/DRRT_Q.jl:2560-2640), written into the edge mirror from the CSR lists the
 * rrtx_extend_candidates* calls wrote (offsets[nq + 1], idx, cost_out, cost_in, hit_out, hit_in; SimpleEdge lists pass
 * the one cost array as cost_out and cost_in).  node_of[j] (int32, nq) is the node index sample j received
 * (rrtx_nodes_append), or a negative value for a sample that was not inserted.  idx_is_batch == 0: idx[e] is a node
 * index (lists against the tree); != 0: idx[e] is a batch position mapped through node_of (the lists of
 * rrtx_extend_candidates_self[_dubins]), and an entry whose mapped value is negative is dropped.
 * ORDER RULE: for j = 0 .. nq-1 with v = node_of[j] >= 0, in that order, and for every surviving entry e of row j in
 * list order, u the near node:
 *   1. the out-edge v -> u, always: distOriginal = cost_out[e], dist = cost_out[e] when hit_out[e] == 0 and +Inf
 *      otherwise (extend links a blocked out-edge with dist = Inf; rrtx_graph_edges_unblock revives it);
 *   2. the in-edge u -> v, only when hit_in[e] == 0: dist = distOriginal = cost_in[e].
 * Edge ids are consecutive from rrtx_graph_edges_count at entry, in exactly that order; they never depend on launch
 * geometry or on the order in which waves finish.  Through every call that reads the mirror (the sweeps, the releases,
 * rrtx_graph_edges_unblock, the cost solvers, rrtx_graph_edges_get) the result is indistinguishable from
 * rrtx_graph_edges_append of those (start, end) pairs in that order, rrtx_graph_edges_set_dist with those original
 * costs and rrtx_graph_edges_block of the out-edges with hit_out != 0.  Duplicate edges and self loops are accepted,
 * as there.  *first_id = the id of the first edge (the count at entry), *n_added = the edges appended (either may be
 * NULL); row_first (nq + 1 int64, may be NULL) = the CSR of every sample's edges relative to *first_id, an empty row
 * for a sample that was not inserted.  nq == 0 or no inserted sample: RRTX_OK, *n_added = 0.
 * Refusals, nothing is appended on any of them (row_first may have been written): RRTX_E_CAPACITY when the extend
 * call produced more entries than cap, or when the mirror would pass the int32 id range; RRTX_E_INVALID for a
 * node_of[j] >= rrtx_nodes_count, for a surviving entry (of an inserted sample) whose near node is outside
 * [0, rrtx_nodes_count) or whose batch position is outside [0, nq), and for offsets out of order or beyond cap.  The
 * verdict is computed on the device, in the pass that counts the edges.
 *
 * rrtx_graph_edges_append_lists_dev: every list array, node_of, n_valid_dev (the count the extend call left on the
 * device, needed_dev; NULL: not checked) and row_first are DEVICE pointers; first_id and n_added are host pointers.  The
 * call waits on the stream ONCE, to read 24 bytes (surviving entries, edges, the verdict); it then grows the mirror if
 * needed (that growth waits once more) and only enqueues the fill.
 * rrtx_graph_edges_append_lists: the same with host arrays (n_valid by value), staged through the path of the
 * host-pointer searches; row_first is a host array or NULL.  This is how a host-pointer caller feeds the self lists.
 * rrtx_graph_edges_append_selected: the same over the lists the last successful rrtx_extend_select or
 * rrtx_extend_select_dubins left in the context (always lists against the tree: idx_is_batch = 0); node_of and
 * row_first are host arrays.  After rrtx_extend_select the one cost column serves as cost_out and cost_in; after
 * rrtx_extend_select_dubins the held cost_out and cost_in columns are read, and the mirror is exactly what
 * rrtx_graph_edges_append_lists of those lists gives.  HOLD RULE: the context
 * records that it holds such lists, with their nq, their count and their cost columns (one or three).  The record survives rrtx_nodes_append[_dev],
 * rrtx_node_cost_set, every rrtx_graph_* call (rrtx_graph_edges_append_lists, which stages into the list workspaces,
 * excepted) and the getters (rrtx_sync, rrtx_get_option, rrtx_stats, rrtx_last_tile_form, the counts, the error text);
 * EVERY other entry point drops it -- the searches, the extend calls, the checks and steers, the sweeps and releases,
 * rrtx_find_new_target*, rrtx_set_option, the obstacle setters -- whether or not it succeeds.  Without a record, or
 * with another nq, the call is RRTX_E_STATE and nothing is appended.
 *
 * rrtx_graph_edges_get reads mirror edges back: the range [first_id, first_id + n) when ids is NULL, else the n edges
 * ids[i] (first_id is then ignored).  start, end, dist (edge.dist, +Inf = blocked) and dist_original may each be NULL.
 * An id or a range outside the mirror is RRTX_E_INVALID and nothing is written.  A host working from
 * rrtx_graph_cost_update_delta resolves the few parent-edge ids it is told about with it. */
int rrtx_graph_edges_append_lists_dev(rrtx_ctx *ctx, int nq, const int64_t *offsets, const int32_t *idx,
                                      const double *cost_out, const double *cost_in, const uint8_t *hit_out,
                                      const uint8_t *hit_in, const int64_t *n_valid_dev, int64_t cap,
                                      const int32_t *node_of, int idx_is_batch, int64_t *first_id, int64_t *n_added,
                                      int64_t *row_first);
int rrtx_graph_edges_append_lists(rrtx_ctx *ctx, int nq, const int64_t *offsets, const int32_t *idx,
                                  const double *cost_out, const double *cost_in, const uint8_t *hit_out,
                                  const uint8_t *hit_in, int64_t n_valid, int64_t cap, const int32_t *node_of,
                                  int idx_is_batch, int64_t *first_id, int64_t *n_added, int64_t *row_first);
int rrtx_graph_edges_append_selected(rrtx_ctx *ctx, int nq, const int32_t *node_of, int64_t *first_id, int64_t *n_added,
                                     int64_t *row_first);
int rrtx_graph_edges_get(rrtx_ctx *ctx, const int32_t *ids, int64_t first_id, int64_t n, int32_t *start, int32_t *end,
                         double *dist, double *dist_original);

/* ---- a robot's new move target ------------------------------------------------- */
/* findNewTarget (R/DRRT_Q.jl:2901-2994) for a batch of robot poses, on the device: kdFindWithinRange around the pose,
 * the edge pose -> neighbour steered and collision-checked for every neighbour, the neighbour with the lowest
 * rrtLMC + edge.dist taken; without a safe one the ball doubles (kdFindMoreWithinRange) until there is one or the ball
 * exceeds r_max (the reference's maxSearchBallRad = dist(S.lowerBounds, S.upperBounds)).  All pointers are host
 * pointers; pose is nq x dim; r0 holds one first radius (r_stride 0) or one per pose (r_stride 1), as in rrtx_nn_radius;
 * lmc is rrtLMC of every node (rrtx_nodes_count doubles) or NULL for the context's own array (rrtx_node_cost_set).
 * Per pose i, independently of the others:
 *   r = r0[i]; k = 1
 *   loop: L = the list rrtx_nn_radius gives at r (root with <=, ghost rule), in ascending node index;
 *         best = +Inf; for e in L: cost = edge.dist of calculateTrajectory for pose_i -> node, blocked = the hit_out byte
 *           of rrtx_extend_candidates[_dubins] for that edge is non-zero (with time it carries !validMove too);
 *           cand = lmc[node] + cost; adopted when !blocked and cand < best (the first of equals wins; NaN and +Inf never);
 *         best != +Inf: status RRTX_TGT_OK, target_idx = node, edge_dist = cost, cost_to_goal = best, radius_used = r,
 *           rounds = k; stop
 *         r = 2 r; r > r_max: status RRTX_TGT_NOT_FOUND, target_idx = -1, edge_dist = cost_to_goal = +Inf,
 *           radius_used = the last radius searched, rounds = k; stop
 *         k += 1
 * The first search is always at r0[i]: clipping it to min(max(hyperBallRad, dist(pose, oldTarget)), r_max) stays with
 * the caller, as in the reference.  Exact, no tolerance: every output is an input value, an index, one rounded fp64
 * addition or r0 * 2^j.  RRTX_E_INVALID unless every r0[i] is finite and positive, r_max is finite and
 * r0[i] >= r_max * 2^-40 (the reference loops forever on r0 = 0); RRTX_E_STATE on an empty tree.
 * The SimpleEdge form needs dim == 3 and no wraps and reads the spheres or the polygons by RRTX_OPT_EXTEND_OBSTACLES;
 * the Dubins form needs dim == 4, honours the wraps and RRTX_OPT_SPACE_HAS_TIME and reads the polygon list.  The
 * neighbour lists stay on the device, in the context-owned buffers of rrtx_extend_select (RRTX_OPT_SELECT_LIST_CAP: a
 * round that produces more grows them and runs once more); per round the host reads three words. */
#define RRTX_TGT_OK 0
#define RRTX_TGT_NOT_FOUND 1
int rrtx_find_new_target(rrtx_ctx *ctx, const double *pose, int nq, const double *r0, int r_stride, double r_max,
                         double robot_radius, const double *lmc, int32_t *target_idx, double *edge_dist,
                         double *cost_to_goal, double *radius_used, int32_t *rounds, uint8_t *status);
int rrtx_find_new_target_dubins(rrtx_ctx *ctx, const double *pose, int nq, const double *r0, int r_stride, double r_max,
                                double robot_radius, double r_min, const double *lmc, int32_t *target_idx,
                                double *edge_dist, double *cost_to_goal, double *radius_used, int32_t *rounds,
                                uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif
