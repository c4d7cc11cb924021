// Device memory of the serving paths: the grow-on-demand buffer every call family keeps one of, the carver that lays a call's arrays
// out inside it, and the two helpers of the tables a model holds between calls (dfree, upload).  Host-side helpers: no kernel here.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace rsys {

// One device buffer that only grows.  reserve() waits for `s` before it replaces the buffer (work in flight may still read the old
// one); the contents are not kept.
struct DevScratch {
  void* p = nullptr; size_t bytes = 0;
  int reserve(size_t need, hipStream_t s) {
    if (need <= bytes) return RSYS_OK;
    HIP_CHECK(hipStreamSynchronize(s));
    if (p) HIP_CHECK(hipFree(p));
    p = nullptr; bytes = 0;
    HIP_CHECK(hipMalloc(&p, need));
    bytes = need;
    return RSYS_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr; bytes = 0;
  }
};

// Sub-buffers of one workspace at 256-byte steps.  Run the same sequence of take() twice: over a null base to learn the size (off),
// then over the buffer.
struct Carve {
  char* p; size_t off = 0;
  template <typename X> X* take(size_t count) {
    X* r = (X*)(p ? p + off : nullptr);
    off += (std::max<size_t>(count, 1) * sizeof(X) + 255) / 256 * 256;
    return r;
  }
};

// `layout` assigns the caller's pointers from the Carve it is given: run over a null base for the size, then, with the buffer grown
// to it, over the buffer
template <class F> int carve_into(DevScratch& ws, hipStream_t s, F&& layout) {
  Carve probe{nullptr};
  layout(probe);
  if (int rc = ws.reserve(probe.off, s)) return rc;
  Carve c{(char*)ws.p};
  layout(c);
  return RSYS_OK;
}

template <typename X> void dfree(X*& p) {
  if (p) hipFree(p);
  p = nullptr;
}

// a new device array with the host's `bytes` in it (at least 4 bytes are allocated: an empty table still has a pointer)
inline int upload(void** dst, const void* src, size_t bytes) {
  HIP_CHECK(hipMalloc(dst, std::max<size_t>(bytes, 4)));
  if (bytes) HIP_CHECK(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  return RSYS_OK;
}

}  // namespace rsys
