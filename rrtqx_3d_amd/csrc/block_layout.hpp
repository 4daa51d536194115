// block_layout.hpp -- packed blocks: several typed arrays in one allocation, described once.
// A block is an ordered list of typed fields (a struct whose members are Field<T>, initialised with take<T> in the order
// they are declared, which is the layout).  The description gives the byte size of the block and every field's address
// under any base: a device workspace or its copy in pinned host memory.  Plain C++: no HIP header is needed, so a host
// program can print the layouts (the ws_self blocks below; the blocks of the host entry points are in rrtx_capi.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rrtx {

template <class T>
struct Field {
  size_t off, count;
  T *in(void *base) const { return reinterpret_cast<T *>(static_cast<char *>(base) + off); }
  // the same address read as U: a vector type of the kernels (double4, float4) over a field declared by its scalars
  template <class U> U *in_as(void *base) const { return reinterpret_cast<U *>(static_cast<char *>(base) + off); }
  size_t bytes() const { return sizeof(T) * count; }
  void to(T *dst, void *base) const { if (dst) std::memcpy(dst, in(base), bytes()); }          // (null: not asked for)
  void from(const T *src, void *base) const { if (src) std::memcpy(in(base), src, bytes()); }  // (null: not given)
};
// `n` elements of T appended to a block of `bytes` bytes, at T's own alignment unless one is given
template <class T>
Field<T> take(size_t &bytes, size_t n, size_t align = alignof(T)) {
  bytes = (bytes + align - 1) & ~(align - 1);
  const Field<T> f{bytes, n};
  bytes += f.bytes();
  return f;
}

// ---- what the four same-batch searches of kernels_self.hip keep in ws_self; `bytes` is what the launcher asks it to hold.
// The sample table and its fp32 shadow are declared by their scalars (four a sample) and read as double4 / float4; they
// come first, so the table sits at the workspace's own alignment and the shadow at a multiple of 32 bytes.  The Dubins
// forms keep the table as four columns of n (x y t theta) and add the shadows' norms and one mark byte a sample
// (dubins = false: those two fields are empty).
struct SelfJoinBlock {              // launch_self_join, launch_self_join_dubins
  size_t n; bool dubins; size_t bytes = 0;
  Field<double> tab = take<double>(bytes, 4 * n);                 // (table_out / columns_out)
  Field<float> shadow = take<float>(bytes, 4 * n), spp = take<float>(bytes, dubins ? n : 0);
  Field<int> count = take<int>(bytes, n + 1);                     // entries per row
  Field<unsigned long long> absmax = take<unsigned long long>(bytes, 1);   // bit pattern of max |q - origin|
  Field<uint8_t> mark = take<uint8_t>(bytes, dubins ? n : 0);
};
// n rows of k slots.  slots_off / rows_off are the "offsets" arrays of the edge kernels (only their last word is read: the
// number of entries); rows = the compact row list, tree_near = the tree column's node indices, row_owner = the rows' own
// indices.  owner_bytes: what ws_owner holds, the owner row of every slot.
struct ClosestSelfBlock {           // launch_closest_self, launch_closest_self_dubins
  size_t n, k; bool dubins; size_t bytes = 0;
  Field<double> tab = take<double>(bytes, 4 * n);
  Field<float> shadow = take<float>(bytes, 4 * n);
  Field<int64_t> slots_off = take<int64_t>(bytes, n + 1), rows_off = take<int64_t>(bytes, n + 1);
  Field<unsigned long long> absmax = take<unsigned long long>(bytes, 1);
  Field<float> spp = take<float>(bytes, dubins ? n : 0);
  Field<int32_t> rows = take<int32_t>(bytes, n), tree_near = take<int32_t>(bytes, n), row_owner = take<int32_t>(bytes, n);
  Field<int32_t> n_rows = take<int32_t>(bytes, 1);
  Field<uint8_t> mark = take<uint8_t>(bytes, dubins ? n : 0);
  size_t slots = n * k, owner_bytes = sizeof(int32_t) * slots;
};

// ---- the packed obstacle tables: what sync_spheres / sync_polygons / sync_polygon_grid (kernels_collide.hip) upload, one
// block and one copy per list, from a host image that is zero-filled before it is packed.  Every field starts on a
// multiple of kTableAlign bytes, what hipMalloc gave each of them while it was a buffer of its own: no vector load of a
// kernel (double4 over meta, float4 over reach_f, the 64-byte sample records) changes its alignment.  The record fields
// are declared by their scalars (SphRec: 4 doubles, SampleSph: 8) and read with in_as.  The slack the separate buffers
// were allocated with is part of its field, unchanged in size: zeros inside the allocation, not what the allocator left.
// Each is one element past the list for the kernels that walk the field:
constexpr size_t kTableAlign = 256;
constexpr size_t kVxySlack = 2;      // doubles, a vertex: the side walks of edges_polygons_kernel, the point kernels, the sweep and Dubins checks
constexpr size_t kSlopeSlack = 1;    // doubles, a side: vslope[vb] of edges_polygons_kernel and of the Dubins check's stage A
constexpr size_t kPathSlack = 3;     // doubles, a row: transform_obs_to_time / edge_hits_moving read rows `before - 1` and `before`
constexpr size_t kYtabSlack = 1;     // doubles: the look-up of points_polygons_flag_kernel (an empty table is still a pointer)
constexpr size_t kSphAuxSlack = 64;  // bytes after radius, thr_in and orig each: points_spheres_kernel, edges_spheres_kernel
struct HostImage {                  // `bytes` zero bytes whose base is aligned like the device allocation's
  std::vector<unsigned char> store;
  void *base;
  explicit HostImage(size_t bytes)
      : store(bytes + kTableAlign, 0), base(store.data() + (-reinterpret_cast<uintptr_t>(store.data()) & (kTableAlign - 1))) {}
};
struct SphereTableBlock {           // sync_spheres: the na spheres in use, list order
  size_t na; size_t bytes = 0;
  Field<double> rec = take<double>(bytes, 4 * na, kTableAlign);           // SphRec: centre, threshold on the squared distance
  Field<double> reach = take<double>(bytes, 4 * na, kTableAlign);         // SphRec: centre, inflated reach
  Field<float> reach_f = take<float>(bytes, 32 * ((na + 7) / 8), kTableAlign);   // fp32 reach, groups of 8, pair-interleaved
  Field<double> sample = take<double>(bytes, 8 * na, kTableAlign);        // SampleSph
  Field<double> radius = take<double>(bytes, na + kSphAuxSlack / sizeof(double), kTableAlign);
  Field<double> thr_in = take<double>(bytes, na + kSphAuxSlack / sizeof(double), kTableAlign);
  Field<int32_t> orig = take<int32_t>(bytes, na + kSphAuxSlack / sizeof(int32_t), kTableAlign);   // list position
};
struct PolygonTableBlock {          // sync_polygons: the na polygons in use, list order; n_ytab entries (0: none)
  size_t na, n_vertices, n_path_rows, n_ytab; size_t bytes = 0;
  Field<double> meta = take<double>(bytes, 4 * na, kTableAlign);          // cx, cy, radius, kind
  Field<int32_t> off = take<int32_t>(bytes, na + 1, kTableAlign);         // vertex CSR
  Field<double> vxy = take<double>(bytes, 2 * n_vertices + kVxySlack, kTableAlign);
  Field<double> vslope = take<double>(bytes, n_vertices + kSlopeSlack, kTableAlign);   // slope of the side that ends at the vertex
  Field<int32_t> orig = take<int32_t>(bytes, na, kTableAlign);            // list position
  Field<double> bbox = take<double>(bytes, 4 * na, kTableAlign);          // box of the vertices: xmin, xmax, ymin, ymax
  Field<double> pbox = take<double>(bytes, 4 * na, kTableAlign);          // box of the centre over the obstacle's path
  Field<double> ytab = take<double>(bytes, n_ytab + kYtabSlack, kTableAlign);   // sorted y of the kind-3 polygons' vertices
  Field<int32_t> path_off = take<int32_t>(bytes, na + 1, kTableAlign);    // path CSR (kinds 6 / 7)
  Field<double> path = take<double>(bytes, 3 * n_path_rows + kPathSlack, kTableAlign);   // rows (dx, dy, t)
};
struct PolygonGridBlock {           // sync_polygon_grid: per cell the first of its items; the packed positions cell by cell
  size_t cells, n_items; size_t bytes = 0;
  Field<int32_t> start = take<int32_t>(bytes, cells + 1, kTableAlign);
  Field<uint16_t> items = take<uint16_t>(bytes, n_items, kTableAlign);    // (its offset depends on `cells` alone)
};

}  // namespace rrtx
