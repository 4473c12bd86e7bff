// Model check of the dynamic-LDS layouts of the PIXEL_VEL kernels (vi_ekf_amd/csrc/viekf_pixvel_lds.hpp), stand-alone on a CPU:
// the header is plain C++17, this program includes nothing else of the library.  For every feature count N = 0 .. 300 (and
// 4096), with nx' / n as viekf_batch_create sets them, PixvelLds, and for M = 1 .. 256 PixvelsLds, are checked for:
//   (a) the regions are pairwise disjoint and lie inside bytes(), each with the size its kernel indexes
//   (b) the rows that are read as pairs or walked by a wave start on even offsets (16-byte boundaries)
//   (c) bytes() equals the formula include/viekf_pixvel.h states
// With arguments "N M" it prints the two byte counts instead (tests/test_pixvel_header_cpu.py compares them with the library's).
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../vi_ekf_amd/csrc/viekf_pixvel_lds.hpp"

namespace {

struct Region { const char* name; long at, size; };   // doubles

long g_cases = 0, g_bad = 0;

void fail(const char* layout, int N, int M, const char* what, const char* r1, const char* r2 = "") {
  if (g_bad++ < 12) std::printf("FAIL %s N=%d M=%d: %s %s %s\n", layout, N, M, what, r1, r2);
}

void check(const char* layout, int N, int M, const std::vector<Region>& regions, long total) {
  g_cases++;
  for (std::size_t i = 0; i < regions.size(); i++) {
    const Region& r = regions[i];
    if (r.at < 0 || r.at + r.size > total) fail(layout, N, M, "region past total:", r.name);
    for (std::size_t j = i + 1; j < regions.size(); j++) {
      const Region& s = regions[j];
      if (r.size && s.size && r.at < s.at + s.size && s.at < r.at + r.size) fail(layout, N, M, "regions overlap:", r.name, s.name);
    }
  }
}

void one(int N) {
  const int nx = 17 + 5 * N, n = 16 + 3 * N, nxs = (nx + 1) & ~1;
  const viekf::PixvelLds L(nxs, n);
  check("PixvelLds", N, 0, {{"xs", L.xs, nxs}, {"W", L.W, 2L * n}, {"K", L.K, 2L * n}, {"lam", L.lam, n}, {"sm", L.sm, 25}}, L.total);
  if (L.W % 2 || L.K % 2) fail("PixvelLds", N, 0, "pairs off a 16-byte boundary", "W/K");
  if (L.bytes() != 8u * (std::size_t)(nxs + 5 * n + 32)) fail("PixvelLds", N, 0, "bytes() differs from the stated formula", "");
  for (int M = 1; M <= viekf::kPixvelsMaxM; M += (M < 8 || N < 20) ? 1 : 13) {
    const viekf::PixvelsLds F(nxs, n, N, M);
    const long nW = F.nW;
    check("PixvelsLds", N, M,
          {{"xs", F.xs, nxs}, {"lam", F.lam, n}, {"D", F.D, N}, {"Pb", F.Pb, 6 * nW}, {"Fc", F.Fc, 3 * nW}, {"sm", F.sm, 25},
           {"Si", F.Si, 4L * M}, {"W", F.W, 2 * nW * M}},
          F.total);
    if (nW < n || nW % 2 || F.Pb % 2 || F.Fc % 2 || F.W % 2 || F.Si % 2) fail("PixvelsLds", N, M, "rows off a 16-byte boundary", "");
    const long even_n = (N + 1) & ~1;
    if (F.bytes() != 8u * (std::size_t)(nxs + nW + even_n + 9 * nW + 32 + 4L * M + 2 * nW * M))
      fail("PixvelsLds", N, M, "bytes() differs from the stated formula", "");
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3) {
    const int N = std::atoi(argv[1]), M = std::atoi(argv[2]);
    const int nx = 17 + 5 * N, n = 16 + 3 * N, nxs = (nx + 1) & ~1;
    std::printf("%zu %zu\n", viekf::PixvelLds(nxs, n).bytes(), viekf::PixvelsLds(nxs, n, N, M).bytes());
    return 0;
  }
  for (int N = 0; N <= 300; N++) one(N);
  one(4096);
  std::printf("%ld layouts checked, %ld failures, max M %d\n", g_cases, g_bad, viekf::kPixvelsMaxM);
  return g_bad ? 1 : 0;
}
