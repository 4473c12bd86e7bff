// viekf_body_lds.hpp -- the dynamic-LDS carve-up of k_update_body_n (viekf_kernels_body.hpp), written ONCE: the kernel takes its
// pointers from the struct, the launch site its byte count (bytes()) and the decision whether the fused route applies at all.
// Plain C++17, no HIP header.  Offsets are in doubles from the start of the dynamic LDS.
#pragma once
#include <cstddef>

namespace viekf {

constexpr int kBodyMaxM = 8;      // VIEKF_BODY_MAX_M (include/viekf_body.h)
constexpr int kBodyCols = 16;     // the body columns of the error state: every body model's H is zero outside them
// Row stride of the panel in doubles.  ds_read_b64 banks per 32-lane half: lane i of a column read sits at dword 34 i, bank
// 2 (17 i mod 32) -- 32 distinct pairs of banks, conflict free; 16 would put lanes i and i + 2 on one bank.
constexpr int kBodyPanelLd = 17;

struct BodyLds {
  int xs;      // [nxs]            the filter's state
  int lam;     // [n]              lambda
  int C;       // [n][17]          the panel P[:, 0:16], row i at C + 17 i (the 17th double of a row is never touched)
  int D;       // [N]              P(rho, rho) of every feature, N = (n - 16) / 3
  int K;       // [M][n][3]        gain of the a-th APPLIED entry (entries that were skipped, gated or guarded take no slot)
  int W;       // [n][M][3]        P H^T of the a-th applied entry, the entries of a row side by side: a column's W of every
               //                  entry is one base address and constant offsets in the trailing pass
  int sm;      // [64]             as GenLds::sm: hcols [0..5], Hc [6..23], res [24..26], ncol [27], Si [28..36], verdict [37]
  int total;
  constexpr BodyLds(int nxs, int n, int M)
      : xs(0), lam(nxs), C(lam + n), D(C + kBodyPanelLd * n), K(D + (n - kBodyCols) / 3), W(K + 3 * n * M), sm(W + 3 * n * M),
        total(sm + 64) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

}  // namespace viekf
