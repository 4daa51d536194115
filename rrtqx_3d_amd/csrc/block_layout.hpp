// block_layout.hpp -- packed blocks: several typed arrays in one allocation, described once.
// A block is an ordered list of typed fields (a struct whose members are Field<T>, initialised with take<T> in the order
// they are declared, which is the layout).  The description gives the byte size of the block and every field's address
// under any base: a device workspace or its copy in pinned host memory.  Plain C++: no HIP header is needed, so a host
// program can print the layouts (the ws_self blocks below; the blocks of the host entry points are in rrtx_capi.hip).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

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

}  // namespace rrtx
