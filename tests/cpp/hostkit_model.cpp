// Host-only model test of vi_ekf_amd/csrc/viekf_hostkit.hpp against tests/cpp/hipstub (built by tests/test_hostkit.py under
// AddressSanitizer + UndefinedBehaviorSanitizer; leaks are counted by the stub itself, not by LeakSanitizer):
//   1. a failing hipMalloc at every position of a handle's set-up   2. more buffers than the old fixed table held
//   3. count == 0                                                   4. reserve: order of the calls, failure
//   5. copy_user: null pointers, the four kinds; check_where
#include <cstdint>
#include <cstdio>

#include "viekf_hostkit.hpp"

static std::string g_err;
int viekf::set_last_error(int code, const std::string& msg) { g_err = msg; return code; }

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    g_checks++;                                                                      \
    if (!(cond)) { g_failed++; std::printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #cond); } \
  } while (0)

static size_t frees_logged() {
  size_t n = 0;
  for (const HipStubCall& c : hip_stub().log) n += c.what == "free";
  return n;
}

// a handle's set-up as the library writes it: K allocations of mixed types, the first failure ends it
constexpr int K = 6;
struct Handle {
  DevOwner own;
  double* a = nullptr; int* b = nullptr; unsigned char* c = nullptr; const uint8_t* d = nullptr; float* e = nullptr; long long* f = nullptr;
  int create(hipStream_t s) {
    int rc = own.alloc(&a, 7);
    if (!rc) rc = own.alloc_zeroed(&b, 5, s);
    if (!rc) rc = own.alloc(&c, 3);
    if (!rc) rc = own.alloc_zeroed(&d, 9, s);
    if (!rc) rc = own.alloc(&e, 1);
    if (!rc) rc = own.alloc(&f, 2);
    return rc;
  }
  const void* ptr(int i) const { const void* p[K] = {a, b, c, d, e, f}; return p[i]; }
};

static void failure_at_every_position() {
  HipStub& st = hip_stub();
  for (int i = 0; i <= K; i++) {   // (i == K: no failure)
    st.reset();
    st.fail_malloc = i;
    Handle h;
    const int rc = h.create(nullptr);
    CHECK(rc == (i < K ? VIEKF_ERR_HIP : VIEKF_OK));
    if (i < K) CHECK(g_err.find("hipMalloc failed") == 0);
    for (int j = 0; j < K; j++) CHECK((h.ptr(j) != nullptr) == (j < i));   // the one it was filling, and all after it, are null
    CHECK(h.own.size() == (size_t)std::min(i, K) && st.live.size() == h.own.size());
    if (i > 1) for (int j = 0; j < 5; j++) CHECK(h.b[j] == 0);              // the zero-filled variant
    h.own.release_all();
    CHECK(st.live.empty() && h.own.size() == 0);
    const size_t n = frees_logged();
    h.own.release_all();
    CHECK(frees_logged() == n);   // the second one frees nothing
  }
}

static void more_than_24_buffers() {
  HipStub& st = hip_stub();
  st.reset();
  DevOwner own;
  double* p[100];
  for (int i = 0; i < 100; i++) {
    CHECK(own.alloc(&p[i], (size_t)i + 1) == VIEKF_OK);
    p[i][i] = 1.0;   // (the last element: inside the allocation)
  }
  CHECK(own.size() == 100 && st.live.size() == 100);
  CHECK(own.free(&p[40]) == VIEKF_OK && p[40] == nullptr && st.live.size() == 99);
  CHECK(own.free(&p[40]) == VIEKF_OK);   // null: nothing to do
  int other = 0;
  int* q = &other;
  CHECK(own.free(&q) == VIEKF_ERR_INVALID && q == &other);   // not this handle's
  own.release_all();
  CHECK(st.live.empty());
}

static void zero_count() {
  HipStub& st = hip_stub();
  st.reset();
  DevOwner own;
  double* p = nullptr;
  char* z = nullptr;
  CHECK(own.alloc(&p, 0) == VIEKF_OK && p != nullptr);
  CHECK(own.alloc_zeroed(&z, 0, nullptr) == VIEKF_OK && z != nullptr && z[0] == 0);
  CHECK(st.log[0].what == "malloc" && st.log[0].bytes >= 1);
  own.release_all();
  CHECK(st.live.empty());
}

static void reserve_grows() {
  HipStub& st = hip_stub();
  hipStream_t stream = reinterpret_cast<hipStream_t>(&st);
  DevOwner own;
  double* p = nullptr;
  size_t cap = 0;
  st.reset();
  CHECK(own.reserve(&p, &cap, 10, stream) == VIEKF_OK && p && cap == 10);
  CHECK(st.log.size() == 1 && st.log[0].what == "malloc" && st.log[0].bytes == 80);   // (nothing to wait for or free yet)
  p[9] = 1.0;
  st.reset();
  CHECK(own.reserve(&p, &cap, 10, stream) == VIEKF_OK && own.reserve(&p, &cap, 3, stream) == VIEKF_OK && own.reserve(&p, &cap, 0, stream) == VIEKF_OK);
  CHECK(st.log.empty() && cap == 10);   // smaller or equal: no call at all
  const void* old = p;
  CHECK(own.reserve(&p, &cap, 11, stream) == VIEKF_OK && cap == 11);
  CHECK(st.log.size() == 3);
  if (st.log.size() == 3) {
    CHECK(st.log[0].what == "sync" && st.log[0].ptr == stream);
    CHECK(st.log[1].what == "free" && st.log[1].ptr == old);
    CHECK(st.log[2].what == "malloc" && st.log[2].ptr == p && st.log[2].bytes == 88);
  }
  CHECK(frees_logged() == 1 && st.live.size() == 1);
  p[10] = 1.0;
  // a larger one whose hipMalloc fails
  st.reset();
  st.fail_malloc = 0;
  CHECK(own.reserve(&p, &cap, 100, stream) == VIEKF_ERR_HIP && p == nullptr && cap == 0);
  CHECK(frees_logged() == 1 && st.live.empty() && own.size() == 0);
  own.release_all();
  CHECK(frees_logged() == 1);   // nothing is freed twice (the stub aborts on one anyway)
  st.reset();
  CHECK(own.reserve(&p, &cap, 4, stream) == VIEKF_OK && cap == 4 && st.log.size() == 1);   // and the handle goes on
  own.release_all();
  CHECK(st.live.empty());
}

static void copies_and_where() {
  HipStub& st = hip_stub();
  st.reset();
  char lib[8] = "library", user[8] = {};
  CHECK(copy_user(nullptr, lib, 8, VIEKF_HOST, Copy::ToUser, nullptr) == VIEKF_OK);
  CHECK(copy_user(lib, nullptr, 8, VIEKF_DEVICE, Copy::FromUser, nullptr) == VIEKF_OK);
  CHECK(st.log.empty());   // a null user pointer: no call
  const struct { viekf_mem where; Copy dir; int kind; } cases[4] = {
      {VIEKF_HOST, Copy::ToUser, hipMemcpyDeviceToHost}, {VIEKF_HOST, Copy::FromUser, hipMemcpyHostToDevice},
      {VIEKF_DEVICE, Copy::ToUser, hipMemcpyDeviceToDevice}, {VIEKF_DEVICE, Copy::FromUser, hipMemcpyDeviceToDevice}};
  for (const auto& c : cases) {
    st.reset();
    const bool to = c.dir == Copy::ToUser;
    CHECK(copy_user(to ? user : lib, to ? lib : user, 8, c.where, c.dir, nullptr) == VIEKF_OK);
    CHECK(st.log.size() == 1 && st.log[0].what == "memcpy" && st.log[0].kind == c.kind && st.log[0].bytes == 8);
  }
  CHECK(check_where(VIEKF_HOST) == VIEKF_OK && check_where(VIEKF_DEVICE) == VIEKF_OK);
  for (int w : {-1, 2, 3, 1000}) {
    g_err.clear();
    CHECK(check_where(static_cast<viekf_mem>(w)) == VIEKF_ERR_INVALID);
    CHECK(g_err == "where must be VIEKF_HOST or VIEKF_DEVICE");
  }
}

int main() {
  failure_at_every_position();
  more_than_24_buffers();
  zero_count();
  reserve_grows();
  copies_and_where();
  std::printf("hostkit model: checks %d failed %d outstanding %zu\n", g_checks, g_failed, hip_stub().live.size());
  if (g_failed || !hip_stub().live.empty()) return 1;
  std::printf("hostkit model: ok\n");
  return 0;
}
