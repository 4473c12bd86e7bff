// viekf_depth_lds.hpp -- the dynamic-LDS carve-up of k_update_depths (viekf_kernels_depth.hpp), written ONCE: the kernel takes its
// pointers from the struct, the launch site its byte count (bytes()) and the decision whether the fused route applies at all.
// Plain C++17, no HIP header.  Offsets are in doubles from the start of the dynamic LDS.
#pragma once
#include <cstddef>

namespace viekf {

constexpr int kDepthsMaxM = 256;   // VIEKF_DEPTHS_MAX_M (include/viekf_depth.h)

struct DepthLds {
  int nW;      // row stride of W: n rounded up to even (a column block of the trailing pass reads 16-byte pairs)
  int xs;      // [nxs]      the filter's state
  int lam;     // [n]        lambda
  int D;       // [N]        P(rho, rho) of every feature, N = (n - 16) / 3
  int bad;     // [2]        the entry's NaN guard (:247): raised by any thread, read by all (no static LDS beside this layout)
  int Si;      // [M]        S^-1 of the a-th APPLIED entry
  int W;       // [M][nW]    row e: first column c_e of the start P for the e-th entry in processing order (loaded up front), then,
               //            rows 0 .. napp - 1, W = P H^T of the a-th applied entry (a <= e: the row it takes has been consumed).
               //            K is one multiply away (K[i] = W[i] * Si) and is not stored.
  int total;
  constexpr DepthLds(int nxs, int n, int M)
      : nW((n + 1) & ~1), xs(0), lam(nxs), D(lam + n), bad((D + (n - 16) / 3 + 1) & ~1), Si(bad + 2), W((Si + M + 1) & ~1), total(W + nW * M) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

}  // namespace viekf
