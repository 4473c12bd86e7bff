// viekf_pixvel_lds.hpp -- the LDS layouts of k_update_pixvel and k_update_pixvels (viekf_kernels_pixvel.hpp), stated once for the
// kernels, their launch site (viekf_capi_pixvel.hpp), viekf_pixvel_lds_bytes / viekf_pixvels_lds_bytes and the host model test (tests/cpp/pixvel_lds_model.cpp, run by tests/test_pixvel_header_cpu.py).  Plain C++:
// no HIP.
#pragma once
#include <cstddef>

namespace viekf {

constexpr int kPixvelsMaxM = 256;

// Offsets in doubles.  nxs = the state's stride (nx rounded up to even), n = 16 + 3 num_features.
struct PixvelLds {
  static constexpr int kSmall = 32;   // Hc [2][9] at 0, residual [2] at 18, S^-1 [4] at 20, the gate's verdict at 24
  int xs;      // [nxs]  the state
  int W;       // [n][2] P H^T
  int K;       // [n][2] W S^-1
  int lam;     // [n]    lambda
  int sm;      // [kSmall]
  int total;
  constexpr PixvelLds(int nxs, int n) : xs(0), W(nxs), K(W + 2 * n), lam(K + 2 * n), sm(lam + n), total(sm + kSmall) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

// k_update_pixvels, the fused route: M entries of one filter, one trailing pass over the lower triangle.  Offsets in doubles.
// N = num_features.  Every row of n doubles is padded to nW = n rounded up to even.
struct PixvelsLds {
  static constexpr int kSmall = 32;   // as PixvelLds
  int nW;      // row length
  int xs;      // [nxs]       the state
  int lam;     // [nW]        lambda
  int D;       // [even(N)]   P(rho, rho) of every feature: fix_depth's edits land here
  int Pb;      // [6][nW]     the columns VEL, B_G of the CURRENT P (rows above the diagonal mirrored in)
  int Fc;      // [3][nW]     the entry's three feature columns of the current P, rebuilt left-looking
  int sm;      // [kSmall]
  int Si;      // [4 M]       S^-1 of every applied entry
  int W;       // [M][2][nW]  W = P H^T of every applied entry, one row per component
  int total;
  constexpr PixvelsLds(int nxs, int n, int N, int M)
      : nW((n + 1) & ~1), xs(0), lam(nxs), D(lam + nW), Pb(D + ((N + 1) & ~1)), Fc(Pb + 6 * nW), sm(Fc + 3 * nW), Si(sm + kSmall),
        W(Si + 4 * M), total(W + 2 * nW * M) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

}  // namespace viekf
