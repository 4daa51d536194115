// fake_hip.cpp -- the simulated HIP runtime (fake_hip.hpp says what it models).  Plain C++17; defines the runtime
// functions the host-only objects of the library need and nothing else of HIP.
#include "fake_hip.hpp"

#include <cxxabi.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <map>
#include <vector>

#if defined(__has_feature)
#if __has_feature(address_sanitizer)
#include <sanitizer/asan_interface.h>
#define FAKEHIP_ASAN 1
#endif
#endif

namespace fakehip {
namespace {

constexpr unsigned char kDevFill = 0xA5, kPinFill = 0x5A;
enum BlockKind { DEV = 0, PINNED = 1, REGISTERED = 2 };
const char *kind_name(int k) { return k == DEV ? "device" : (k == PINNED ? "pinned" : "registered"); }

struct Block {
  char *p;
  size_t n;
  int kind;
  unsigned long id;                    // the number of the hipMalloc / hipHostMalloc / hipHostRegister call
  std::vector<unsigned char> written;  // device blocks: one byte per byte
};

enum RangeMode { R_READ, R_WRITE, R_UPDATE, R_SCRATCH, R_MAPPED, R_READ_ANY };
struct Range { const char *p; size_t n; int mode; std::string what; };

enum OpKind { OP_COPY, OP_MEMSET, OP_KERNEL };
struct Op {
  int kind = OP_COPY;
  unsigned long seq = 0;
  std::string label;                   // the driver's case at the call
  char *dst = nullptr;
  const char *src = nullptr;
  size_t n = 0;
  hipMemcpyKind mk = hipMemcpyDefault;
  int value = 0;
  bool host_pageable = false;          // the host side of an H2D / D2H copy is pageable
  bool has_snap = false;
  std::vector<char> snap;              // pageable H2D: the source as it was at the call
  std::string kernel;
  std::vector<Range> ranges;
  std::vector<std::function<void()>> scripts;
};

struct KernelRec { std::string name; long launches = 0; const char *cite = nullptr; Contract fn = nullptr; bool looked_up = false; };
struct ContractRec { std::string part; const char *cite; Contract fn; };

struct State {
  std::map<uintptr_t, Block> blocks;
  std::map<hipStream_t, std::deque<Op>> queues;
  std::map<const void *, KernelRec> kernels;
  std::vector<ContractRec> contracts;
  unsigned long n_alloc = 0, n_op = 0;
  long n_findings = 0, n_copies = 0, n_bad_launches = 0;
  hipError_t last_error = hipSuccess;
  std::string label, known;
  long n_known = 0, n_known_now = 0;
  bool strict = false;
  // the launch configuration between __hipPushCallConfiguration and __hipPopCallConfiguration
  dim3 cfg_grid, cfg_block; size_t cfg_shmem = 0; hipStream_t cfg_stream = nullptr;
};
State &S() {
  static State *s = [] {
    State *st = new State();
    const char *e = std::getenv("FAKEHIP_STRICT");
    st->strict = e && e[0] == '1';
    return st;
  }();
  return *s;
}

Block *containing(const void *p, size_t n) {   // the live block [p, p + n) lies inside, of any kind
  auto &b = S().blocks;
  const uintptr_t a = (uintptr_t)p;
  auto it = b.upper_bound(a);
  if (it == b.begin()) return nullptr;
  --it;
  Block &k = it->second;
  return (a >= (uintptr_t)k.p && a + n <= (uintptr_t)k.p + k.n) ? &k : nullptr;
}
Block *touching(const void *p) {               // the live block the address p lies in (or one byte past)
  auto &b = S().blocks;
  const uintptr_t a = (uintptr_t)p;
  auto it = b.upper_bound(a);
  if (it == b.begin()) return nullptr;
  --it;
  Block &k = it->second;
  return (a >= (uintptr_t)k.p && a <= (uintptr_t)k.p + k.n) ? &k : nullptr;
}
std::string where(const void *p, size_t n) {
  char buf[200];
  if (Block *k = touching(p)) {
    const size_t off = (size_t)((const char *)p - k->p);
    std::snprintf(buf, sizeof(buf), "%zu bytes at offset %zu of %s block #%lu (%zu bytes): %zu past its end", n, off,
                  kind_name(k->kind), k->id, k->n, off + n - k->n);
  } else {
    std::snprintf(buf, sizeof(buf), "%zu bytes at %p, in no live block", n, p);
  }
  return buf;
}
const char *copy_kind(hipMemcpyKind k) {
  return k == hipMemcpyHostToDevice ? "H2D" : k == hipMemcpyDeviceToHost ? "D2H" : k == hipMemcpyDeviceToDevice ? "D2D" : "H2H";
}
std::string op_name(const Op &o) {
  char buf[300];
  if (o.kind == OP_COPY) std::snprintf(buf, sizeof(buf), "copy %s #%lu of %zu bytes [%s]", copy_kind(o.mk), o.seq, o.n, o.label.c_str());
  else if (o.kind == OP_MEMSET) std::snprintf(buf, sizeof(buf), "memset #%lu of %zu bytes [%s]", o.seq, o.n, o.label.c_str());
  else std::snprintf(buf, sizeof(buf), "launch #%lu of %s [%s]", o.seq, o.kernel.c_str(), o.label.c_str());
  return buf;
}

// a device range of an operation: inside one live device block?  (finding otherwise)
Block *device_range(const Op &o, const void *p, size_t n, const char *side, const char *when) {
  Block *k = containing(p, n);
  if (k && k->kind == DEV) return k;
  finding("%s: %s %s: %s", op_name(o).c_str(), side, when, where(p, n).c_str());
  return nullptr;
}
bool read_shadow(const Op &o, Block *k, const char *p, size_t n, const char *side) {
  const size_t off = (size_t)(p - k->p);
  for (size_t i = 0; i < n; ++i)
    if (!k->written[off + i]) {
      finding("%s: %s reads a device byte nothing wrote: block #%lu (hipMalloc call %lu, %zu bytes), first at offset %zu "
              "(byte %zu of the range)", op_name(o).c_str(), side, k->id, k->id, k->n, off + i, i);
      return false;
    }
  return true;
}
void mark_written(Block *k, const char *p, size_t n) {
  std::fill_n(k->written.begin() + (p - k->p), n, (unsigned char)1);
}
bool host_pinned(const void *p, size_t n) {
  Block *k = containing(p, n);
  return k && (k->kind == PINNED || k->kind == REGISTERED);
}
bool poisoned(const void *p, size_t n) {
#ifdef FAKEHIP_ASAN
  return __asan_region_is_poisoned(const_cast<void *>(p), n) != nullptr;
#else
  (void)p; (void)n;
  return false;
#endif
}

void exec_copy(Op &o) {
  S().n_copies += 1;
  if (o.mk == hipMemcpyHostToDevice) {
    Block *d = device_range(o, o.dst, o.n, "destination", "at execution");
    const char *from = o.src;
    if (o.host_pageable) {
      if (o.has_snap && !S().strict) from = o.snap.data();
      else if (poisoned(o.src, o.n)) {
        finding("%s: strict: the pageable source is no longer alive when the copy executes", op_name(o).c_str());
        from = o.has_snap ? o.snap.data() : nullptr;
      } else if (o.has_snap && std::memcmp(o.src, o.snap.data(), o.n) != 0) {
        finding("%s: strict: the pageable source changed between the call and the execution", op_name(o).c_str());
      }
    } else if (!host_pinned(o.src, o.n)) {
      finding("%s: the pinned source is gone at execution: %s", op_name(o).c_str(), where(o.src, o.n).c_str());
      from = nullptr;
    }
    if (d && from) { std::memcpy(o.dst, from, o.n); mark_written(d, o.dst, o.n); }
  } else if (o.mk == hipMemcpyDeviceToHost) {
    Block *s = device_range(o, o.src, o.n, "source", "at execution");
    if (s) read_shadow(o, s, o.src, o.n, "source");
    bool ok = s != nullptr;
    if (o.host_pageable) {
      if (S().strict && poisoned(o.dst, o.n)) {
        finding("%s: strict: the pageable destination is no longer alive when the copy executes", op_name(o).c_str());
        ok = false;
      }
    } else if (!host_pinned(o.dst, o.n)) {
      finding("%s: the pinned destination is gone at execution: %s", op_name(o).c_str(), where(o.dst, o.n).c_str());
      ok = false;
    }
    if (ok) std::memcpy(o.dst, o.src, o.n);
  } else if (o.mk == hipMemcpyDeviceToDevice) {
    Block *s = device_range(o, o.src, o.n, "source", "at execution");
    Block *d = device_range(o, o.dst, o.n, "destination", "at execution");
    if (s) read_shadow(o, s, o.src, o.n, "source");
    if (s && d) {
      std::memmove(o.dst, o.src, o.n);
      std::copy_n(s->written.begin() + (o.src - s->p), o.n, d->written.begin() + (o.dst - d->p));   // the shadow goes across
    }
  } else {
    std::memmove(o.dst, o.src, o.n);
  }
}

void exec_kernel(Op &o) {
  bool in_bounds = true;
  for (const Range &r : o.ranges) {
    Block *k = containing(r.p, r.n);
    const bool want_dev = r.mode != R_MAPPED;
    if (!k || (want_dev ? k->kind != DEV : k->kind != PINNED)) {
      finding("%s: argument %s at execution: %s", op_name(o).c_str(), r.what.c_str(), where(r.p, r.n).c_str());
      in_bounds = false;
      continue;
    }
    if (r.mode == R_READ || r.mode == R_UPDATE) read_shadow(o, k, r.p, r.n, ("argument " + r.what).c_str());
  }
  for (const Range &r : o.ranges)
    if (r.mode == R_WRITE || r.mode == R_UPDATE || r.mode == R_SCRATCH)
      if (Block *k = containing(r.p, r.n)) if (k->kind == DEV) mark_written(k, r.p, r.n);
  if (in_bounds)                       // (a script stores through the kernel's pointers: not past a block's end)
    for (auto &fn : o.scripts) fn();
}

void exec(Op &o) {
  if (o.kind == OP_COPY) exec_copy(o);
  else if (o.kind == OP_MEMSET) {
    if (Block *d = device_range(o, o.dst, o.n, "destination", "at execution")) {
      std::memset(o.dst, o.value, o.n);
      mark_written(d, o.dst, o.n);
    }
  } else exec_kernel(o);
}
void drain(hipStream_t st) {
  auto &q = S().queues[st];
  while (!q.empty()) {
    Op o = std::move(q.front());
    q.pop_front();
    exec(o);
  }
}
void drain_all() {
  std::vector<hipStream_t> sts;
  for (auto &kv : S().queues) sts.push_back(kv.first);
  for (hipStream_t st : sts) drain(st);
}
bool overlaps(const void *p, size_t n, const char *lo, const char *hi) {
  return p && n && (const char *)p < hi && (const char *)p + n > lo;
}
// the first queued operation that names a byte of [lo, hi)
const Op *queued_naming(const char *lo, const char *hi) {
  for (auto &kv : S().queues)
    for (const Op &o : kv.second) {
      if (o.kind != OP_KERNEL && (overlaps(o.dst, o.n, lo, hi) || (o.kind == OP_COPY && !o.has_snap && overlaps(o.src, o.n, lo, hi)))) return &o;
      for (const Range &r : o.ranges) if (overlaps(r.p, r.n, lo, hi)) return &o;
    }
  return nullptr;
}

Op new_op(int kind) {
  Op o;
  o.kind = kind;
  o.seq = ++S().n_op;
  o.label = S().label;
  return o;
}

// queue (or, for the synchronous form, execute after everything queued) one copy
hipError_t copy(void *dst, const void *src, size_t n, hipMemcpyKind mk, hipStream_t st, bool sync) {
  if (n == 0) return hipSuccess;
  if (!dst || !src) return S().last_error = hipErrorInvalidValue;
  if (mk == hipMemcpyDefault) {
    Block *d = containing(dst, 1), *s = containing(src, 1);
    const bool dd = d && d->kind == DEV, sd = s && s->kind == DEV;
    mk = dd ? (sd ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice) : (sd ? hipMemcpyDeviceToHost : hipMemcpyHostToHost);
  }
  Op o = new_op(OP_COPY);
  o.dst = (char *)dst; o.src = (const char *)src; o.n = n; o.mk = mk;
  bool wait = sync;
  if (mk == hipMemcpyHostToDevice) {
    device_range(o, dst, n, "destination", "at the call");
    if (Block *h = containing(src, 1)) if (h->kind == DEV) finding("%s: the host source is device memory", op_name(o).c_str());
    o.host_pageable = !host_pinned(src, n);
    if (o.host_pageable) {             // documented: the pageable source is read before the call returns
      o.snap.assign((const char *)src, (const char *)src + n);
      o.has_snap = true;
    }
  } else if (mk == hipMemcpyDeviceToHost) {
    device_range(o, src, n, "source", "at the call");
    if (Block *h = containing(dst, 1)) if (h->kind == DEV) finding("%s: the host destination is device memory", op_name(o).c_str());
    o.host_pageable = !host_pinned(dst, n);
    // documented: a copy to pageable memory has arrived when the call returns (strict: it is deferred like a pinned one)
    if (o.host_pageable && !S().strict) wait = true;
    if (o.host_pageable) {             // the caller's array has room for the bytes (the sanitizer looks at every one)
      volatile char *c = (volatile char *)dst;
      for (size_t i = 0; i < n; i += 1) c[i] = (char)0xEE;
    }
  } else if (mk == hipMemcpyDeviceToDevice) {
    device_range(o, src, n, "source", "at the call");
    device_range(o, dst, n, "destination", "at the call");
  }
  if (sync) {
    // the synchronous calls are not ordered against a non-blocking stream: what is queued must not name their ranges
    if (const Op *q = queued_naming((const char *)dst, (const char *)dst + n))
      finding("%s: synchronous, but %s is still queued on its destination", op_name(o).c_str(), op_name(*q).c_str());
    drain_all();
    exec(o);
    return hipSuccess;
  }
  S().queues[st].push_back(std::move(o));
  if (wait) drain(st);
  return hipSuccess;
}

hipError_t memset_op(void *dst, int value, size_t n, hipStream_t st, bool sync) {
  if (n == 0) return hipSuccess;
  Op o = new_op(OP_MEMSET);
  o.dst = (char *)dst; o.n = n; o.value = value;
  device_range(o, dst, n, "destination", "at the call");
  if (sync) {
    if (const Op *q = queued_naming((const char *)dst, (const char *)dst + n))
      finding("%s: synchronous, but %s is still queued on its destination", op_name(o).c_str(), op_name(*q).c_str());
    drain_all();
    exec(o);
  } else S().queues[st].push_back(std::move(o));
  return hipSuccess;
}

hipError_t add_block(void **out, size_t n, int kind, unsigned char fill) {
  if (!out) return hipErrorInvalidValue;
  *out = nullptr;
  if (n == 0) return hipSuccess;
  Block b;
  b.p = new char[n];                   // exactly n bytes: the sanitizer's red zones make every extent byte-exact
  std::memset(b.p, fill, n);
  b.n = n; b.kind = kind; b.id = ++S().n_alloc;
  if (kind == DEV) b.written.assign(n, 0);
  *out = b.p;
  S().blocks[(uintptr_t)b.p] = std::move(b);
  return hipSuccess;
}
hipError_t remove_block(void *p, int kind, const char *fn) {
  if (!p) return hipSuccess;
  auto it = S().blocks.find((uintptr_t)p);
  if (it == S().blocks.end() || it->second.kind != kind) {
    finding("%s(%p): not the start of a live %s block", fn, p, kind_name(kind));
    return S().last_error = hipErrorInvalidValue;
  }
  if (kind != DEV)                     // hipFree waits for the device; nothing says that of pinned memory
    if (const Op *q = queued_naming(it->second.p, it->second.p + it->second.n))
      finding("%s of %s block #%lu (%zu bytes) while %s still names it", fn, kind_name(kind), it->second.id, it->second.n,
              op_name(*q).c_str());
  drain_all();
  it = S().blocks.find((uintptr_t)p);
  delete[] it->second.p;               // (the sanitizer's quarantine then catches a later use of a stale view)
  S().blocks.erase(it);
  return hipSuccess;
}

std::string demangle(const char *name) {
  int status = 0;
  char *d = abi::__cxa_demangle(name, nullptr, nullptr, &status);
  std::string out = (status == 0 && d) ? d : name;
  std::free(d);
  return out;
}

}  // namespace

// ---- what contracts and drivers call ---------------------------------------------------------------------------------
struct Launch::Impl { Op *op; };

static void declare(Launch &L, const void *p, size_t bytes, const char *what, bool null_ok, int mode) {
  Op &o = *L.impl->op;
  if (!p) {
    if (!null_ok && bytes) finding("%s: argument %s is null", op_name(o).c_str(), what);
    return;
  }
  if (!bytes) return;
  Block *k = containing(p, bytes);
  const bool want_dev = mode != R_MAPPED;
  if (!k || (want_dev ? k->kind != DEV : k->kind != PINNED))
    finding("%s: argument %s at the launch: %s", op_name(o).c_str(), what, where(p, bytes).c_str());
  o.ranges.push_back(Range{(const char *)p, bytes, mode, what});
}
void Launch::reads(const void *p, size_t n, const char *what, bool null_ok) { declare(*this, p, n, what, null_ok, R_READ); }
void Launch::writes(const void *p, size_t n, const char *what, bool null_ok) { declare(*this, p, n, what, null_ok, R_WRITE); }
void Launch::updates(const void *p, size_t n, const char *what, bool null_ok) { declare(*this, p, n, what, null_ok, R_UPDATE); }
void Launch::reads_unchecked(const void *p, size_t n, const char *what, bool null_ok) { declare(*this, p, n, what, null_ok, R_READ_ANY); }
void Launch::scratch(const void *p, size_t n, const char *what, bool null_ok) { declare(*this, p, n, what, null_ok, R_SCRATCH); }
void Launch::writes_mapped(const void *p, size_t n, const char *what) { declare(*this, p, n, what, false, R_MAPPED); }
void Launch::script(std::function<void()> fn) { impl->op->scripts.push_back(std::move(fn)); }

void contract(const char *name_part, const char *cite, Contract fn) { S().contracts.push_back(ContractRec{name_part, cite, fn}); }

void finding(const char *fmt, ...) {
  char buf[900];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (!S().known.empty() && std::strstr(buf, S().known.c_str())) {
    S().n_known_now += 1;
    S().n_known += 1;
    std::printf("KNOWN %s   (during: %s)\n", buf, S().label.c_str());
  } else {
    S().n_findings += 1;
    // (after a first finding the flow may run on whatever the workspaces held: the first lines are the ones to read)
    if (S().n_findings <= 200) std::printf("FINDING %s   (during: %s)\n", buf, S().label.c_str());
    if (S().n_findings == 200) std::printf("FINDING (further findings are counted, not printed)\n");
  }
  std::fflush(stdout);
}
void known_begin(const std::string &part) { S().known = part; S().n_known_now = 0; }
void known_end() {
  const std::string part = S().known;
  S().known.clear();
  if (S().n_known_now != 1) finding("the known finding \"%s\" came %ld times, not once", part.c_str(), S().n_known_now);
}
long findings() { return S().n_findings; }
bool strict() { return S().strict; }
void context(const std::string &label) { S().label = label; }

int report() {
  drain_all();
  std::map<std::string, std::pair<long, const char *>> by_name;
  for (auto &kv : S().kernels)
    if (kv.second.launches) {
      auto &e = by_name[kv.second.name];
      e.first += kv.second.launches;
      e.second = kv.second.cite;
    }
  for (auto &kv : by_name) std::printf("LAUNCH %ld %s   <- %s\n", kv.second.first, kv.first.c_str(), kv.second.second ? kv.second.second : "NO CONTRACT");
  std::printf("COPIES %ld\n", S().n_copies);
  std::printf("LIVE_BLOCKS %zu\n", S().blocks.size());
  std::printf("KNOWN_FINDINGS %ld\n", S().n_known);
  std::printf("FINDINGS %ld\n", S().n_findings);
  std::fflush(stdout);
  return S().n_findings ? 3 : 0;
}

}  // namespace fakehip

using namespace fakehip;

// ---- the runtime functions the objects need ----------------------------------------------------------------------------
extern "C" {

void **__hipRegisterFatBinary(const void *) { static void *handle[1] = {nullptr}; return handle; }
void __hipUnregisterFatBinary(void **) {}
void __hipRegisterFunction(void **, const void *host_function, char *, const char *device_name, unsigned, void *, void *,
                           dim3 *, dim3 *, int *) {
  S().kernels[host_function].name = demangle(device_name);
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
  S().cfg_grid = grid; S().cfg_block = block; S().cfg_shmem = shmem; S().cfg_stream = stream;
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3 *grid, dim3 *block, size_t *shmem, hipStream_t *stream) {
  *grid = S().cfg_grid; *block = S().cfg_block; *shmem = S().cfg_shmem; *stream = S().cfg_stream;
  return hipSuccess;
}

hipError_t hipLaunchKernel(const void *function, dim3 grid, dim3 block, void **args, size_t, hipStream_t stream) {
  KernelRec &k = S().kernels[function];
  if (k.name.empty()) k.name = "(a function no module registered)";
  if (!k.looked_up) {
    k.looked_up = true;
    for (const ContractRec &c : S().contracts)
      if (k.name.find(c.part) != std::string::npos) { k.fn = c.fn; k.cite = c.cite; break; }
  }
  Op o = new_op(OP_KERNEL);
  o.kernel = k.name;
  const unsigned long long threads = (unsigned long long)block.x * block.y * block.z;
  if (grid.x == 0 || grid.y == 0 || grid.z == 0 || threads == 0 || threads > 1024) {
    S().n_bad_launches += 1;
    finding("%s: invalid configuration: grid (%u, %u, %u), block (%u, %u, %u)", op_name(o).c_str(), grid.x, grid.y, grid.z,
            block.x, block.y, block.z);
    return S().last_error = hipErrorInvalidConfiguration;
  }
  k.launches += 1;
  if (!k.fn) {
    if (k.launches == 1) finding("NOCONTRACT %s: launched on a driven path without a contract", k.name.c_str());
    return hipSuccess;
  }
  Launch::Impl impl{&o};
  Launch L{k.name.c_str(), args, grid, block, &impl};
  k.fn(L);
  S().queues[stream].push_back(std::move(o));
  return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t n) { return add_block(p, n, DEV, kDevFill); }
hipError_t hipFree(void *p) { return remove_block(p, DEV, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned) { return add_block(p, n, PINNED, kPinFill); }
hipError_t hipHostFree(void *p) { return remove_block(p, PINNED, "hipHostFree"); }
hipError_t hipHostRegister(void *p, size_t n, unsigned) {
  if (!p || !n) return S().last_error = hipErrorInvalidValue;
  if (containing(p, 1)) return S().last_error = hipErrorHostMemoryAlreadyRegistered;
  Block b;
  b.p = (char *)p; b.n = n; b.kind = REGISTERED; b.id = ++S().n_alloc;
  S().blocks[(uintptr_t)p] = std::move(b);
  return hipSuccess;
}
hipError_t hipHostUnregister(void *p) {
  auto it = S().blocks.find((uintptr_t)p);
  if (it == S().blocks.end() || it->second.kind != REGISTERED) return S().last_error = hipErrorHostMemoryNotRegistered;
  if (const Op *q = queued_naming(it->second.p, it->second.p + it->second.n))
    finding("hipHostUnregister of range #%lu (%zu bytes) while %s still names it", it->second.id, it->second.n, op_name(*q).c_str());
  S().blocks.erase(it);
  return hipSuccess;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind) { return copy(dst, src, n, kind, nullptr, true); }
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t st) { return copy(dst, src, n, kind, st, false); }
hipError_t hipMemset(void *dst, int value, size_t n) { return memset_op(dst, value, n, nullptr, true); }
hipError_t hipMemsetAsync(void *dst, int value, size_t n, hipStream_t st) { return memset_op(dst, value, n, st, false); }

hipError_t hipStreamCreateWithFlags(hipStream_t *st, unsigned) { *st = reinterpret_cast<hipStream_t>(new char[1]); return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t st) {
  drain(st);
  S().queues.erase(st);
  delete[] reinterpret_cast<char *>(st);
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t st) { drain(st); return hipSuccess; }

hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : (S().last_error = hipErrorInvalidDevice); }
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipGetLastError(void) { const hipError_t e = S().last_error; S().last_error = hipSuccess; return e; }
const char *hipGetErrorString(hipError_t e) {
  switch (e) {
    case hipSuccess: return "no error";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorInvalidConfiguration: return "invalid configuration argument";
    case hipErrorOutOfMemory: return "out of memory";
    default: return "an error of the simulated runtime";
  }
}

hipError_t hipEventCreate(hipEvent_t *e) { *e = reinterpret_cast<hipEvent_t>(new char[1]); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { delete[] reinterpret_cast<char *>(e); return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { drain_all(); return hipSuccess; }
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) { *ms = 0.f; return hipSuccess; }

}  // extern "C"
