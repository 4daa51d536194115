// contracts.hpp -- what the drivers tell the kernel contracts (contracts.cpp) about the scene they have set up, and the
// values the scripts store where the host reads a result back.
#pragma once

#include <cstdint>

namespace hostsim {

struct Scene {
  int dim = 3;
  long long n_nodes = 0;
  int sph_na = 0;                              // spheres in use
  int poly_na = 0, poly_nv = 0, poly_rows = 0; // polygons in use, their vertices, the rows of their paths
  // the script of the range search's last kernel: `total` entries, dealt over the samples as evenly as they go (the
  // first total % nq samples hold one more), every entry a valid node; nearest_miss_every > 0: every such sample gets
  // the nearest index -1, which sends the host form to its fallback
  long long total = 0;
  int nearest_miss_every = 0;
};
extern Scene scene;

void register_contracts();

}  // namespace hostsim
