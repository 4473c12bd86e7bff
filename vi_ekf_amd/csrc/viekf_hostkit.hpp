// viekf_hostkit.hpp -- the host plumbing every handle of the C ABI shares (batch, KLT tracker, simulator, frame intake, node
// graph): the error return, the check of `where`, the copies to and from a caller's array, and DevOwner, the device
// allocations of one handle.  Host code only -- no kernel, no launch, nothing __device__: tests/cpp/hostkit_model.cpp compiles
// it with a plain C++ compiler against a stub of the HIP header.  The pinned ring, the streams and Staged are not in here.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/viekf.h"
#include "viekf_host.hpp"

namespace {

inline int fail(int code, const std::string& msg) { return viekf::set_last_error(code, msg); }

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      return fail(VIEKF_ERR_HIP, std::string(#expr) + " failed: " + hipGetErrorString(e_));            \
  } while (0)

inline int check_where(viekf_mem where) {
  if (where != VIEKF_HOST && where != VIEKF_DEVICE) return fail(VIEKF_ERR_INVALID, "where must be VIEKF_HOST or VIEKF_DEVICE");
  return VIEKF_OK;
}

// One array between the library's device memory and the caller's (`where` says which side the caller's lives on), queued on
// `s`.  ToUser: dst is the caller's; FromUser: src is.  A null caller's pointer is an array that was not asked for / given.
enum class Copy { ToUser, FromUser };
inline int copy_user(void* dst, const void* src, size_t bytes, viekf_mem where, Copy dir, hipStream_t s) {
  if (!(dir == Copy::ToUser ? dst : src)) return VIEKF_OK;
  const hipMemcpyKind kind = where == VIEKF_DEVICE ? hipMemcpyDeviceToDevice
                                                   : (dir == Copy::ToUser ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice);
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, s));
  return VIEKF_OK;
}

// The device allocations of one handle: whatever alloc / reserve hands out is freed by release_all, which a destroy function
// calls after it has set the device and waited for the work that may still use the buffers.  Counts are in elements of T.
class DevOwner {
 public:
  DevOwner() = default;
  DevOwner(const DevOwner&) = delete;
  DevOwner& operator=(const DevOwner&) = delete;

  // max(count * sizeof(T), 1) bytes.  On failure *p stays null and nothing is recorded.
  template <typename T>
  int alloc(T** p, size_t count) { return take(p, count, false, nullptr); }
  // ... zero-filled on `s` (in stream order: the caller synchronises before the host relies on it)
  template <typename T>
  int alloc_zeroed(T** p, size_t count, hipStream_t s) { return take(p, count, true, s); }

  // Grow-only buffer of at least `count` elements: nothing when it is large enough; otherwise wait for `s` (the old buffer
  // may be in use there), free it, allocate.  Pointer and capacity are null and 0 in between, and stay so on failure.
  template <typename T>
  int reserve(T** p, size_t* capacity, size_t count, hipStream_t s) {
    if (count <= *capacity) return VIEKF_OK;
    if (*p) {
      HIP_TRY(hipStreamSynchronize(s));
      if (int rc = free(p)) return rc;
    }
    *capacity = 0;
    if (int rc = alloc(p, count)) return rc;
    *capacity = count;
    return VIEKF_OK;
  }

  // one buffer the handle is replacing (null: nothing to do)
  template <typename T>
  int free(T** p) {
    if (!*p) return VIEKF_OK;
    void* q = const_cast<void*>(static_cast<const void*>(*p));
    const auto it = std::find(bufs_.begin(), bufs_.end(), q);
    if (it == bufs_.end()) return fail(VIEKF_ERR_INVALID, "DevOwner::free: not a buffer of this handle");
    bufs_.erase(it);
    *p = nullptr;
    HIP_TRY(hipFree(q));
    return VIEKF_OK;
  }

  void release_all() {
    for (void* q : bufs_) (void)hipFree(q);
    bufs_.clear();
  }

  size_t size() const { return bufs_.size(); }

 private:
  template <typename T>
  int take(T** p, size_t count, bool zero, hipStream_t s) {
    *p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 1);
    bufs_.reserve(bufs_.size() + 1);   // (so that recording the buffer below cannot fail)
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(VIEKF_ERR_HIP, std::string("hipMalloc failed: ") + hipGetErrorString(e));
    if (zero && (e = hipMemsetAsync(q, 0, bytes, s)) != hipSuccess) {
      (void)hipFree(q);
      return fail(VIEKF_ERR_HIP, std::string("hipMemsetAsync failed: ") + hipGetErrorString(e));
    }
    bufs_.push_back(q);
    *p = static_cast<T*>(q);
    return VIEKF_OK;
  }

  std::vector<void*> bufs_;
};

}  // namespace
