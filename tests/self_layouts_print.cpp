// Prints the ws_self layouts of kernels_self.hip's four launchers: for every (nq, k) pair given on the command line one
// line per field, "<block> <nq> <k> <field> <offset>", and the block's size as the field "bytes".  Plain C++: includes
// the block descriptions and nothing of HIP (tests/test_self_layouts.py builds and runs it).
// With "tables" as the first argument: the three obstacle-table blocks for every (na, vertices, path rows, ytab entries)
// given, one line per field, "<block> <na> <nv> <rows> <nytab> <field> <offset> <count> <element size>", "bytes" likewise
// (count 0), and the slack constants once.  The host image of every block must come aligned and zero-filled, and every field's first
// and last element (slack included) is written in it: what the sanitized build is for.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../rrtqx_3d_amd/csrc/block_layout.hpp"

using namespace rrtx;

static void put(const char *block, size_t nq, size_t k, const char *field, size_t value) {
  std::printf("%s %zu %zu %s %zu\n", block, nq, k, field, value);
}
#define PUT(block, B, field) put(block, nq, k, #field, (B).field.off)

template <class T>
static void touch(const Field<T> &f, void *base) {
  if (f.count == 0) return;
  f.in(base)[0] = (T)1;
  f.in(base)[f.count - 1] = (T)1;
}
#define TPUT(block, B, field)                                                                                       \
  (std::printf("%s %zu %zu %zu %zu %s %zu %zu %zu\n", block, na, nv, rows, nytab, #field, (B).field.off, (B).field.count, \
               sizeof(*(B).field.in(nullptr))),                                                                   \
   touch((B).field, image.base))
static int fresh(const char *block, const HostImage &image, size_t bytes) {   // aligned, and all zero before the packing
  size_t nonzero = reinterpret_cast<uintptr_t>(image.base) % kTableAlign;
  for (size_t i = 0; i < bytes; ++i) nonzero += static_cast<const unsigned char *>(image.base)[i] != 0;
  if (nonzero) std::fprintf(stderr, "%s: image not aligned or not zero-filled\n", block);
  return nonzero != 0;
}

static int tables(int argc, char **argv) {
  std::printf("slack vxy %zu vslope %zu path %zu ytab %zu sph_aux_bytes %zu align %zu\n", kVxySlack, kSlopeSlack, kPathSlack,
              kYtabSlack, kSphAuxSlack, kTableAlign);
  int bad = 0;
  for (int i = 2; i + 3 < argc; i += 4) {
    const size_t na = std::strtoull(argv[i], nullptr, 10), nv = std::strtoull(argv[i + 1], nullptr, 10),
                 rows = std::strtoull(argv[i + 2], nullptr, 10), nytab = std::strtoull(argv[i + 3], nullptr, 10);
    {
      const SphereTableBlock S{na};
      const HostImage image(S.bytes);
      bad |= fresh("spheres", image, S.bytes);
      TPUT("spheres", S, rec); TPUT("spheres", S, reach); TPUT("spheres", S, reach_f); TPUT("spheres", S, sample);
      TPUT("spheres", S, radius); TPUT("spheres", S, thr_in); TPUT("spheres", S, orig);
      std::printf("spheres %zu %zu %zu %zu bytes %zu 0 1\n", na, nv, rows, nytab, S.bytes);
    }
    {
      const PolygonTableBlock P{na, nv, rows, nytab};
      const HostImage image(P.bytes);
      bad |= fresh("polygons", image, P.bytes);
      TPUT("polygons", P, meta); TPUT("polygons", P, off); TPUT("polygons", P, vxy); TPUT("polygons", P, vslope);
      TPUT("polygons", P, orig); TPUT("polygons", P, bbox); TPUT("polygons", P, pbox); TPUT("polygons", P, ytab);
      TPUT("polygons", P, path_off); TPUT("polygons", P, path);
      std::printf("polygons %zu %zu %zu %zu bytes %zu 0 1\n", na, nv, rows, nytab, P.bytes);
    }
    {
      const PolygonGridBlock G{na, nv};      // (cells = na, items = nv: any two counts do)
      const HostImage image(G.bytes);
      bad |= fresh("grid", image, G.bytes);
      TPUT("grid", G, start); TPUT("grid", G, items);
      std::printf("grid %zu %zu %zu %zu bytes %zu 0 1\n", na, nv, rows, nytab, G.bytes);
    }
  }
  return bad;
}

int main(int argc, char **argv) {
  if (argc > 1 && std::strcmp(argv[1], "tables") == 0) return tables(argc, argv);
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
