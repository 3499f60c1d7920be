// common.h - error plumbing and small device helpers shared by every translation unit.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../include/diffab_hip.h"

namespace diffab {

void set_error(const char* fmt, ...);

#define DIFFAB_REQUIRE(cond, code, ...)  \
  do {                                   \
    if (!(cond)) {                       \
      ::diffab::set_error(__VA_ARGS__);  \
      return (code);                     \
    }                                    \
  } while (0)

#define DIFFAB_HIP_CHECK(expr)                                                              \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      ::diffab::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return DIFFAB_ERR_HIP;                                                                \
    }                                                                                       \
  } while (0)

#define DIFFAB_LAUNCH_CHECK()                                                               \
  do {                                                                                      \
    hipError_t e_ = hipGetLastError();                                                      \
    if (e_ != hipSuccess) {                                                                 \
      ::diffab::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
      return DIFFAB_ERR_HIP;                                                                \
    }                                                                                       \
  } while (0)

static inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// (The library never calls getenv; the kernel variants that were measured and not adopted, and the environment switches used to A/B
// them, live under experiments/ as patches on top of these sources.)

// Cross-stream ordering guard, first statement of every stream-taking entry point (include/diffab_hip.h, "Streams").  OFF by default since
// round 6 (the miscompute it worked around was the v_pk_*_f32 op_sel:[0,1] hazard, removed from every kernel: profiles/r06_lanes_48_63.md);
// then the constructor is one relaxed atomic load.  When switched on (diffab_set_stream_guard(1)): work the library enqueued on a DIFFERENT
// stream before is ordered in front of this call (hipEventRecord on the previous stream + hipStreamWaitEvent on this one).
class StreamOrder {
 public:
  explicit StreamOrder(void* stream);
  ~StreamOrder();
  StreamOrder(const StreamOrder&) = delete;
  StreamOrder& operator=(const StreamOrder&) = delete;

 private:
  int dev_;
};

// Operand alignment (include/diffab_hip.h, "Operand alignment"): an entry whose kernels read or write a data operand with 16-byte vector
// accesses refuses it here - on the host, among its argument checks, before anything is enqueued - when the pointer is not 16-byte
// aligned.  A NULL operand (an optional one left out) passes.  The message names the entry and the operand.
struct Operand {
  const char* name;
  const void* p;
};
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline int require_aligned16(const char* who, std::initializer_list<Operand> ops) {
  for (const Operand& o : ops)
    DIFFAB_REQUIRE(aligned16(o.p), DIFFAB_ERR_ARG, "%s: operand %s must be 16-byte aligned (see \"Operand alignment\" in diffab_hip.h)", who,
                   o.name);
  return DIFFAB_OK;
}

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over the caller's workspace: a null base gives null pointers and the size.  Carves are 256-B aligned; align =
// sizeof(float) packs float buffers back to back (the training tape and the backward's workspace, whose offsets pick kernels).
struct Carver {
  char* base;
  size_t align, off = 0;
  explicit Carver(void* p, size_t align_ = 256) : base(static_cast<char*>(p)), align(align_) {}
  template <typename T>
  T* take(size_t n) {
    off = align_up(off, align);
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += n * sizeof(T);
    return r;
  }
  size_t bytes() const { return align_up(off, align); }
};

}  // namespace diffab
