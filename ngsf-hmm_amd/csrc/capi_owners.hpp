// capi_owners.hpp -- owners of what the C ABI layer takes from the HIP runtime: device buffers,
// pinned host buffers, events and streams.  Plain move-only structs that release in their
// destructors and convert to the raw pointer / event / stream, so that a kernel launch or a
// hipMemcpy reads the same with them.  An early return releases a call's temporaries; deleting the
// handle releases everything it holds (capi_internal.hpp: the order of its members).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "../../include/nghmm.h"

namespace capi {

void set_error(const char* fmt, ...);

// n elements (at least one) of device memory behind a raw pointer: what the owners below hold,
// and the fast-mode state's own pointers (kernels_fast.hpp)
template <typename T>
int dev_alloc(T** p, size_t n) {
  if (n == 0) n = 1;
  hipError_t e = hipMalloc((void**)p, n * sizeof(T));
  if (e != hipSuccess) {
    set_error("hipMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
    return NGHMM_ERR_NOMEM;
  }
  return NGHMM_OK;
}

// what the owners share: one raw value, null when empty, handed over by a move
template <typename H>
struct Owner {
  H p = nullptr;
  Owner() = default;
  Owner(Owner&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
  Owner(const Owner&) = delete;
  Owner& operator=(const Owner&) = delete;
  operator H() const { return p; }
};

template <typename T>
struct DevBuf : Owner<T*> {
  bool borrowed = false;  // p is somebody else's (a replica's view of its parent's data arrays)
  DevBuf() = default;
  DevBuf(DevBuf&&) = default;
  ~DevBuf() { reset(); }
  void reset() {
    if (this->p && !borrowed) (void)hipFree(this->p);
    this->p = nullptr;
    borrowed = false;
  }
  int alloc(size_t n) {
    reset();
    return dev_alloc(&this->p, n);
  }
  void borrow(T* q) {
    reset();
    this->p = q;
    borrowed = true;
  }
};

// the same in pinned host memory
template <typename T>
struct PinBuf : Owner<T*> {
  PinBuf() = default;
  PinBuf(PinBuf&&) = default;
  ~PinBuf() { reset(); }
  void reset() {
    if (this->p) (void)hipHostFree(this->p);
    this->p = nullptr;
  }
  int alloc(size_t n) {
    reset();
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&this->p), n * sizeof(T), hipHostMallocDefault);
    if (e != hipSuccess) {
      this->p = nullptr;
      set_error("hipHostMalloc of %zu bytes failed: %s", n * sizeof(T), hipGetErrorString(e));
      return NGHMM_ERR_HIP;
    }
    return NGHMM_OK;
  }
  // to and from the callers of nghmm_alloc_host / nghmm_free_host, who hold the raw pointer
  T* release() { return std::exchange(this->p, nullptr); }
  void adopt(T* q) {
    reset();
    this->p = q;
  }
};

// a buffer that grows on demand: after reserve(n) it holds at least n elements, exactly n when it
// had to grow; its contents are not kept.  A failed reserve leaves it empty (null, capacity 0).
template <typename Buf>
struct Scratch : Buf {
  size_t cap = 0;
  void reset() {
    Buf::reset();
    cap = 0;
  }
  int reserve(size_t n) {
    if (n <= cap) return NGHMM_OK;
    reset();
    int rc;
    if ((rc = this->alloc(n))) return rc;
    cap = n;
    return NGHMM_OK;
  }
};
template <typename T>
using DevScratch = Scratch<DevBuf<T>>;
template <typename T>
using PinScratch = Scratch<PinBuf<T>>;

struct Event : Owner<hipEvent_t> {
  Event() = default;
  Event(Event&&) = default;
  ~Event() {
    if (p) (void)hipEventDestroy(p);
  }
  int create(unsigned flags = hipEventDefault) {
    hipError_t e = hipEventCreateWithFlags(&p, flags);
    if (e != hipSuccess) {
      p = nullptr;
      set_error("hipEventCreateWithFlags failed: %s", hipGetErrorString(e));
      return NGHMM_ERR_HIP;
    }
    return NGHMM_OK;
  }
};

// a non-blocking stream (every stream of this layer is one)
struct Stream : Owner<hipStream_t> {
  Stream() = default;
  Stream(Stream&&) = default;
  ~Stream() {
    if (p) (void)hipStreamDestroy(p);
  }
  int create() {
    hipError_t e = hipStreamCreateWithFlags(&p, hipStreamNonBlocking);
    if (e != hipSuccess) {
      p = nullptr;
      set_error("hipStreamCreateWithFlags failed: %s", hipGetErrorString(e));
      return NGHMM_ERR_HIP;
    }
    return NGHMM_OK;
  }
};

}  // namespace capi
