// fake_hip.hpp -- a simulated HIP runtime for the host layer of librrtx_hip.so (tests/test_host_layer_sim.py).
//
// The library's sources are compiled for the host alone and linked against fake_hip.cpp instead of the HIP runtime, so
// that rrtx_capi.hip and the launchers run with no GPU, under the address and undefined-behaviour sanitizers.  Kernels
// do not run.  What the runtime models is what a GPU hides:
//   * device memory: a heap block of exactly the bytes asked for, filled with a pattern, with a per-byte `written` shadow;
//   * stream order: copies, memsets and launches are queued per stream and execute when the host waits;
//   * pinned against pageable host memory, as documented for HIP (FAKEHIP_STRICT=1 defers pageable copies as well);
//   * every range an operation names is looked up in the table of live blocks at the call and again at execution;
//   * a copy that reads a device byte nothing wrote is a finding.
// A kernel is known by the name __hipRegisterFunction delivered for its host stub.  A driver registers a CONTRACT per
// kernel: from the argument array of the launch, which device ranges the kernel may read and write, and a SCRIPT: host
// code run at execution that stores chosen values through the kernel's pointers (a count, CSR offsets), which is what
// lets the host flow go on where it reads a result back.  A launch of a kernel without a contract is reported.
//
// The contracts are a reading of the kernels, not the kernels: this checks the host layer, not what a kernel reads.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <functional>
#include <string>

namespace fakehip {

// What a contract sees of one launch.  reads / writes / updates declare a device range of the kernel; they are checked
// against the live blocks at once and again, with the written shadow, when the launch executes.
struct Launch {
  const char *kernel;          // demangled name
  void **args;                 // the argument array of hipLaunchKernel: args[i] points at the i-th argument's value
  dim3 grid, block;
  struct Impl;
  Impl *impl;

  template <class T> T arg(int i) const { T v; std::memcpy(&v, args[i], sizeof(T)); return v; }
  template <class T> T *ptr(int i) const { return arg<T *>(i); }
  long long threads() const { return (long long)grid.x * grid.y * grid.z * block.x * block.y * block.z; }

  // `what` names the argument in a finding.  A null pointer is a finding unless null_ok; zero bytes declare nothing.
  void reads(const void *p, size_t bytes, const char *what, bool null_ok = false);
  void writes(const void *p, size_t bytes, const char *what, bool null_ok = false);
  void updates(const void *p, size_t bytes, const char *what, bool null_ok = false);   // read, then written (atomics)
  // a range the kernel may load from before it knows how much of it holds entries, and does not use beyond them: the
  // extent is checked, the written shadow is not
  void reads_unchecked(const void *p, size_t bytes, const char *what, bool null_ok = false);
  // the range is the kernel's scratch: it may read there what it, or an earlier launch, wrote or did not (no shadow check)
  void scratch(const void *p, size_t bytes, const char *what, bool null_ok = false);
  // a pinned, host-mapped word the kernel writes
  void writes_mapped(const void *p, size_t bytes, const char *what);
  // host code run when the launch executes, after its declared writes have been marked
  void script(std::function<void()> fn);
};

using Contract = void (*)(Launch &);
// `name_part`: the first registered contract whose name_part occurs in the demangled kernel name is the kernel's.
// `cite`: where the kernel's index arithmetic was read (file:lines), printed with the launch counts.
void contract(const char *name_part, const char *cite, Contract fn);

void finding(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
long findings();
bool strict();                 // FAKEHIP_STRICT=1
// a label for the findings that follow (the driver's current case)
void context(const std::string &label);
// Between the two calls a finding whose text contains `part` is printed as KNOWN and not counted: for a finding that has
// been looked at, is recorded in DESIGN.md 4.9 and is not to be mended.  It must then come exactly once, or known_end
// reports that instead -- a known finding that stops coming is stale.
void known_begin(const std::string &part);
void known_end();
// Prints one "LAUNCH <count> <kernel>" line per kernel launched, "COPIES <n>", "FINDINGS <n>"; returns the driver's
// exit status: 0 clean, 3 findings.
int report();

}  // namespace fakehip
