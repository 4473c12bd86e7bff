// A stub of <hip/hip_runtime.h> for host-only tests of vi_ekf_amd/csrc/viekf_hostkit.hpp (tests/cpp/hostkit_model.cpp): "device"
// memory is malloc's, every call is logged, the n-th hipMalloc can be made to fail, and the number of outstanding allocations
// is kept here (the test's leak check; a free of a pointer that is not outstanding aborts).  Nothing of the real runtime.
#pragma once
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0, hipErrorOutOfMemory = 2;
typedef struct hipStub_stream* hipStream_t;
enum hipMemcpyKind { hipMemcpyHostToHost = 0, hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2, hipMemcpyDeviceToDevice = 3 };

struct HipStubCall {
  std::string what;       // "malloc", "free", "memset", "memcpy", "sync"
  const void* ptr;        // the allocation / destination / stream
  size_t bytes;
  int kind;               // memcpy only
};

struct HipStub {
  std::vector<HipStubCall> log;
  std::set<void*> live;   // outstanding allocations
  long mallocs = 0;       // hipMalloc calls so far, failed ones included
  long fail_malloc = -1;  // the hipMalloc call (counted from 0) that fails; -1: none
  void reset() { log.clear(); mallocs = 0; fail_malloc = -1; }
};
inline HipStub& hip_stub() { static HipStub s; return s; }

inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stub: out of memory"; }

inline hipError_t hipMalloc(void** p, size_t bytes) {
  HipStub& s = hip_stub();
  if (s.mallocs++ == s.fail_malloc) return hipErrorOutOfMemory;
  if (bytes == 0) { std::fprintf(stderr, "hipstub: hipMalloc of 0 bytes\n"); std::abort(); }
  *p = std::malloc(bytes);   // (exactly `bytes`: AddressSanitizer sees a write past them)
  s.live.insert(*p);
  s.log.push_back({"malloc", *p, bytes, 0});
  return hipSuccess;
}

inline hipError_t hipFree(void* p) {
  HipStub& s = hip_stub();
  if (!s.live.erase(p)) { std::fprintf(stderr, "hipstub: hipFree of a pointer that is not outstanding\n"); std::abort(); }
  s.log.push_back({"free", p, 0, 0});
  std::free(p);
  return hipSuccess;
}

inline hipError_t hipMemsetAsync(void* p, int v, size_t bytes, hipStream_t) {
  hip_stub().log.push_back({"memset", p, bytes, 0});
  std::memset(p, v, bytes);
  return hipSuccess;
}

inline hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
  hip_stub().log.push_back({"memcpy", dst, bytes, (int)kind});
  std::memcpy(dst, src, bytes);
  return hipSuccess;
}

inline hipError_t hipStreamSynchronize(hipStream_t s) {
  hip_stub().log.push_back({"sync", s, 0, 0});
  return hipSuccess;
}
