// viekf_staging.hpp -- how a call's host-pointer arguments reach the device and its results come back: a bump allocator over
// one device staging region per batch (plus, under viekf_batch_set_async, a pinned ring), and the call-scoped Staged, in which
// an entry point names each of its arrays, with its element count, exactly once.
#pragma once
#include <cstring>

#include "viekf_batch.hpp"

namespace {

constexpr size_t kZeroCopyBytes = 4u << 20;

size_t stage_size(size_t bytes) { return bytes + 256; }

// bump allocator over one device staging region (host-pointer calls only)
int stage_begin(viekf_batch* b, size_t need) {
  need += 4096;
  if (int rc = b->own.reserve(&b->d_stage, &b->stage_bytes, need, b->stream)) return rc;
  b->stage_used = 0;
  if (b->async_host) {
    // A pinned RING on the host side (the copies out of it run later, in stream order) and a ring on the device side too: the
    // previous call's kernel may still be reading its staged arguments, and although the next call's copy is ordered behind it
    // on the stream, a ring lets the copy engine run ahead.  Both wrap after a stream synchronise.
    const size_t ring = std::max<size_t>(64 * need, 8u << 20);   // (a wrap drains the stream: 64 calls of this size apart)
    if (ring > b->pin_bytes) {
      HIP_TRY(hipStreamSynchronize(b->stream));
      if (b->h_pin) HIP_TRY(hipHostFree(b->h_pin));
      b->h_pin = nullptr; b->pin_bytes = 0;
      HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&b->h_pin), ring, hipHostMallocMapped));
      void* dp = nullptr;
      HIP_TRY(hipHostGetDevicePointer(&dp, b->h_pin, 0));
      b->d_pin = static_cast<char*>(dp);
      b->pin_bytes = ring; b->pin_used = 0;
    }
    if (b->pin_used + need > b->pin_bytes) {   // wrap: everything queued so far has to have left the ring
      HIP_TRY(hipStreamSynchronize(b->stream));
      b->pin_used = 0;
    }
  }
  return VIEKF_OK;
}

void* stage_take(viekf_batch* b, size_t bytes) {
  const size_t off = (b->stage_used + 255) & ~size_t(255);
  b->stage_used = off + bytes;
  return b->d_stage + off;
}

// returns a device pointer for an input array: the pointer itself (device) or a staged copy (host)
template <typename Tp>
int in_ptr(viekf_batch* b, const Tp* src, size_t count, viekf_mem where, const Tp** out) {
  if (!src) { *out = nullptr; return VIEKF_OK; }
  if (where == VIEKF_DEVICE) { *out = src; return VIEKF_OK; }
  Tp* d = static_cast<Tp*>(stage_take(b, count * sizeof(Tp)));
  const void* from = src;
  if (b->async_host) {   // the caller's array may change as soon as the call returns: its bytes go through pinned memory now
    const size_t bytes = count * sizeof(Tp), off = (b->pin_used + 255) & ~size_t(255);
    if (off + bytes > b->pin_bytes) return fail(VIEKF_ERR_INVALID, "async staging overflow");   // (stage_begin sized it)
    std::memcpy(b->h_pin + off, src, bytes);
    b->pin_used = off + bytes;
    from = b->h_pin + off;
    // The kernels read their arguments (an IMU sample and a dt per filter; a frame's pixels and slots: about 1 KB per filter)
    // straight out of the pinned ring: every workgroup fetches its own few hundred bytes across the host link in its prologue,
    // which costs the launch less than copy commands between the kernels cost the stream (each one a switch of engines).
    if (bytes <= kZeroCopyBytes) { *out = reinterpret_cast<const Tp*>(b->d_pin + off); return VIEKF_OK; }
  }
  HIP_TRY(hipMemcpyAsync(d, from, count * sizeof(Tp), hipMemcpyHostToDevice, b->stream));
  *out = d;
  return VIEKF_OK;
}

// One array of a call, for Staged::begin: In (read by the kernels) or Out (written by them), the caller's pointer -- nullptr
// for an optional array that is not given -- its element count, and where the device pointer the kernels get is put.
template <typename T>
struct In { const T* src; size_t count; const T** dev; bool host_only; };
template <typename T>
struct Out { T* dst; size_t count; T** dev; bool zeroed; };
template <typename T> In<T> in(const T* src, size_t count, const T** dev) { return {src, count, dev, false}; }
// an array the entry point built itself: on the host whatever the call's `where`
template <typename T> In<T> in_host(const T* src, size_t count, const T** dev) { return {src, count, dev, true}; }
template <typename T> Out<T> out(T* dst, size_t count, T** dev) { return {dst, count, dev, false}; }
// ... zero-filled before the launch (a kernel that writes only part of it)
template <typename T> Out<T> out_zeroed(T* dst, size_t count, T** dev) { return {dst, count, dev, true}; }

// The staged arrays of ONE call.  begin() takes every array of the call, inputs first: VIEKF_DEVICE arrays come back as they
// are; for host arrays it sizes the staging region (and the pinned ring) from the very list it is given, queues the inputs'
// copies in the order listed and sets the outputs' device addresses.  finish() after the launches: the outputs' copies back,
// in the order listed, and the synchronise a host caller is owed.
class Staged {
 public:
  Staged(viekf_batch* b, viekf_mem where) : b_(b), where_(where) {}

  template <typename... A>
  int begin(A... arrays) {
    if (where_ == VIEKF_HOST || (host_only(arrays) || ...))
      if (int rc = stage_begin(b_, (stage_size(bytes(arrays)) + ...))) return rc;
    int rc = VIEKF_OK;
    ((rc = rc ? rc : put(arrays)), ...);
    return rc;
  }

  // may_skip_sync: the routes that queue work only -- nothing to hand back -- return without waiting under viekf_batch_set_async
  int finish(bool may_skip_sync = false) {
    if (where_ != VIEKF_HOST) return VIEKF_OK;
    for (int i = 0; i < nback_; i++)
      HIP_TRY(hipMemcpyAsync(back_[i].host, back_[i].dev, back_[i].bytes, hipMemcpyDeviceToHost, b_->stream));
    if (!(may_skip_sync && b_->async_host && nback_ == 0)) HIP_TRY(hipStreamSynchronize(b_->stream));
    return VIEKF_OK;
  }

 private:
  template <typename T> static size_t bytes(const In<T>& a) { return a.count * sizeof(T); }
  template <typename T> static size_t bytes(const Out<T>& a) { return a.count * sizeof(T); }
  template <typename T> static bool host_only(const In<T>& a) { return a.host_only; }
  template <typename T> static bool host_only(const Out<T>&) { return false; }

  template <typename T>
  int put(const In<T>& a) { return in_ptr(b_, a.src, a.count, a.host_only ? VIEKF_HOST : where_, a.dev); }
  template <typename T>
  int put(const Out<T>& a) {
    *a.dev = a.dst;
    if (!a.dst || where_ == VIEKF_DEVICE) return VIEKF_OK;
    if (nback_ == kMaxOut) return fail(VIEKF_ERR_INVALID, "more staged outputs than Staged keeps track of");
    *a.dev = static_cast<T*>(stage_take(b_, bytes(a)));
    if (a.zeroed) HIP_TRY(hipMemsetAsync(*a.dev, 0, bytes(a), b_->stream));
    back_[nback_++] = {a.dst, *a.dev, bytes(a)};
    return VIEKF_OK;
  }

  static constexpr int kMaxOut = 5;   // (viekf_frame_intake hands back five arrays)
  viekf_batch* b_;
  viekf_mem where_;
  struct Back { void* host; const void* dev; size_t bytes; } back_[kMaxOut];
  int nback_ = 0;
};

}  // namespace
