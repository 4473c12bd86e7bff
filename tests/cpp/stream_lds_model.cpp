// Model check of the dynamic-LDS layouts of the streaming-side kernels (vi_ekf_amd/csrc/viekf_stream_lds.hpp), stand-alone on a
// CPU: the header is plain C++17, this program includes nothing else of the library.  For every feature count N = 0 .. 512, with
// nx / nxs / n as viekf_batch_create sets them, and for several sizes of BodyCtx (odd multiples of 4 bytes among them), every
// struct is checked for three things:
//   (a) its regions are pairwise disjoint and lie inside bytes()
//   (b) every region of doubles starts on an 8-byte boundary
//   (c) bytes() equals the RECORDED FORMULA: the expression the launch site of the kernel used before the layouts were stated
//       once, written out literally below -- a launch must ask for exactly the bytes it always asked for.
// The size of a region is what its kernel indexes (the comments of the header's fields).
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../vi_ekf_amd/csrc/viekf_stream_lds.hpp"

namespace {

struct Region { const char* name; std::size_t at, size; bool doubles; };   // bytes

long g_cases = 0, g_bad = 0;

void fail(const char* layout, int N, std::size_t ctx, const char* what, const char* r1, const char* r2 = "") {
  if (g_bad++ < 12) std::printf("FAIL %s N=%d ctx_bytes=%zu: %s %s %s\n", layout, N, ctx, what, r1, r2);
}

void check(const char* layout, int N, std::size_t ctx, const std::vector<Region>& regions, std::size_t bytes, std::size_t recorded) {
  g_cases++;
  for (std::size_t i = 0; i < regions.size(); i++) {
    const Region& r = regions[i];
    if (r.at + r.size > bytes) fail(layout, N, ctx, "region past bytes():", r.name);
    if (r.doubles && r.at % 8 != 0) fail(layout, N, ctx, "doubles off an 8-byte boundary:", r.name);
    if (!r.doubles && r.at % 4 != 0) fail(layout, N, ctx, "words off a 4-byte boundary:", r.name);
    for (std::size_t j = i + 1; j < regions.size(); j++) {
      const Region& s = regions[j];
      if (r.size && s.size && r.at < s.at + s.size && s.at < r.at + r.size) fail(layout, N, ctx, "regions overlap:", r.name, s.name);
    }
  }
  if (bytes != recorded) fail(layout, N, ctx, "bytes() differs from the recorded formula", "");
}

Region dbl(const char* name, int at, std::size_t count) { return {name, sizeof(double) * (std::size_t)at, sizeof(double) * count, true}; }

}  // namespace

int main() {
  using namespace viekf;
  const std::size_t ctx_sizes[] = {440, 436, 444, 4, 8, 12, 1028};   // 440 = today's BodyCtx (55 doubles)
  for (int N = 0; N <= 512; N++) {
    const int nx = 17 + 5 * N, nxs = (nx + 1) & ~1, n = 16 + 3 * N;
    const std::size_t un = (std::size_t)n, unxs = (std::size_t)nxs;
    for (std::size_t cb : ctx_sizes) {
      for (int mf = 0; mf < 2; mf++) {
        const PropLds L(nxs, cb, N, mf != 0);
        // the launch sites of k_propagate_stream: lds_propagate(b), and "+ 9 N + 2 doubles" for the matrix-core instance
        std::size_t recorded = sizeof(double) * (std::size_t)(nxs + 256 + 96 + 256 + 256 + 96 + 256 + 256 + 16) + cb + 16;
        if (mf) recorded += sizeof(double) * (9 * (std::size_t)N + 2);
        check(mf ? "PropLds(mf)" : "PropLds", N, cb,
              {dbl("xs", L.xs, unxs), dbl("Abb", L.Abb, 256), dbl("Gb", L.Gb, 96), dbl("Phibb", L.Phibb, 256), dbl("Mbb", L.Mbb, 256),
               dbl("Gdb", L.Gdb, 96), dbl("Pbb", L.Pbb, 256), dbl("T16", L.T16, 256), dbl("xdb", L.xdb, 16),
               {"ctx", sizeof(double) * (std::size_t)L.ctx, cb, true}, dbl("Dl", L.Dl, mf ? 9 * (std::size_t)N : 0)},
              L.bytes(), recorded);
      }
      const XdotLds X(nxs, cb);
      check("XdotLds", N, cb,
            {dbl("xs", X.xs, unxs), dbl("Abb", X.Abb, 256), dbl("Gb", X.Gb, 96), dbl("xdb", X.xdb, 16),
             {"ctx", sizeof(double) * (std::size_t)X.ctx, cb, true}},
            X.bytes(), sizeof(double) * (std::size_t)(nxs + 256 + 96 + 16) + cb + 16);   // viekf_batch_eval_xdot
    }
    const UpdLds U(nxs, n);
    check("UpdLds", N, 0, {dbl("xs", U.xs, unxs), dbl("W", U.W, 2 * un), dbl("K", U.K, 2 * un), dbl("lam", U.lam, un), dbl("sm", U.sm, 32)},
          U.bytes(), sizeof(double) * (std::size_t)(nxs + 5 * n + 32));                   // lds_update(b)
    const GenLds G(nxs, n);
    check("GenLds", N, 0, {dbl("xs", G.xs, unxs), dbl("W", G.W, 3 * un), dbl("K", G.K, 3 * un), dbl("lam", G.lam, un), dbl("sm", G.sm, 64)},
          G.bytes(), sizeof(double) * (std::size_t)(nxs + 7 * n + 64));                   // viekf_batch_update
    const KeepLds Kp(n);
    check("KeepLds", N, 0,
          {{"colbuf", Kp.colbuf, sizeof(double) * un, true}, {"srcrow", Kp.srcrow, sizeof(int) * un, false}, {"cnt", Kp.cnt, sizeof(int), false}},
          Kp.bytes(), sizeof(double) * (std::size_t)n + sizeof(int) * (std::size_t)(n + 4));   // viekf_batch_keep_features, viekf_frame_update
  }
  std::printf("cases %ld failures %ld\n", g_cases, g_bad);
  if (g_bad) { std::printf("stream lds model: FAILED\n"); return 1; }
  std::printf("stream lds model: ok\n");
  return 0;
}
