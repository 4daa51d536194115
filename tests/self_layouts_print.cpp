// Prints the ws_self layouts of kernels_self.hip's four launchers: for every (nq, k) pair given on the command line one
// line per field, "<block> <nq> <k> <field> <offset>", and the block's size as the field "bytes".  Plain C++: includes
// the block descriptions and nothing of HIP (tests/test_self_layouts.py builds and runs it).
#include <cstdio>
#include <cstdlib>

#include "../rrtqx_3d_amd/csrc/block_layout.hpp"

using namespace rrtx;

static void put(const char *block, size_t nq, size_t k, const char *field, size_t value) {
  std::printf("%s %zu %zu %s %zu\n", block, nq, k, field, value);
}
#define PUT(block, B, field) put(block, nq, k, #field, (B).field.off)

int main(int argc, char **argv) {
  for (int i = 1; i + 1 < argc; i += 2) {
    const size_t nq = std::strtoull(argv[i], nullptr, 10), k = std::strtoull(argv[i + 1], nullptr, 10);
    for (int dubins = 0; dubins < 2; ++dubins) {
      const char *join = dubins ? "self_join_dubins" : "self_join", *closest = dubins ? "closest_self_dubins" : "closest_self";
      const SelfJoinBlock J{nq, dubins != 0};
      PUT(join, J, tab); PUT(join, J, shadow); PUT(join, J, spp); PUT(join, J, count); PUT(join, J, absmax); PUT(join, J, mark);
      put(join, nq, k, "bytes", J.bytes);
      const ClosestSelfBlock C{nq, k, dubins != 0};
      PUT(closest, C, tab); PUT(closest, C, shadow); PUT(closest, C, slots_off); PUT(closest, C, rows_off);
      PUT(closest, C, absmax); PUT(closest, C, spp); PUT(closest, C, rows); PUT(closest, C, tree_near);
      PUT(closest, C, row_owner); PUT(closest, C, n_rows); PUT(closest, C, mark);
      put(closest, nq, k, "bytes", C.bytes);
      put(closest, nq, k, "owner_bytes", C.owner_bytes);
    }
  }
  return 0;
}
