// viekf_stream_lds.hpp -- the dynamic-LDS carve-ups of the streaming-side kernels, each written ONCE: the kernel takes its
// pointers from the struct, the launch site its byte count (bytes()), so the two cannot drift apart.  Plain C++17, no HIP header:
// a host compiler includes it too (tests/cpp/stream_lds_model.cpp checks every struct for every N).  Offsets are in doubles
// from the start of the dynamic LDS unless a struct says otherwise; the size of each region stands beside its offset.
// sizeof(BodyCtx) cannot be seen from here: the caller passes it in (ctx_bytes).
#pragma once
#include <cstddef>

namespace viekf {

// k_propagate_stream<T, MF> (viekf_kernels_stream.hpp).  mf: the matrix-core instance keeps the Phi_ff blocks in LDS as well (Dl).
struct PropLds {
  static constexpr int kSlackBytes = 16;   // unused bytes past the last region (the launch has always asked for them)
  int xs;      // [nxs]
  int Abb;     // 16x16 row-major
  int Gb;      // 16x6
  int Phibb;   // 16x16
  int Mbb;     // 16x16
  int Gdb;     // 16x6
  int Pbb;     // 16x16 row-major copy of P_bb
  int T16;     // 16x16 scratch
  int xdb;     // 16
  int ctx;     // BodyCtx, ctx_bytes bytes
  int Dl;      // [N][9] Phi_ff blocks (MF only), on the next 8-byte boundary past ctx; followed by 2 spare doubles
  int dl_doubles;   // 9 N + 2 with mf, 0 without
  std::size_t ctx_bytes;
  constexpr PropLds(int nxs, std::size_t ctx_bytes_, int N, bool mf)
      : xs(0), Abb(nxs), Gb(Abb + 256), Phibb(Gb + 96), Mbb(Phibb + 256), Gdb(Mbb + 256), Pbb(Gdb + 96), T16(Pbb + 256),
        xdb(T16 + 256), ctx(xdb + 16), Dl(ctx + (int)((ctx_bytes_ + 7) / 8)), dl_doubles(mf ? 9 * N + 2 : 0), ctx_bytes(ctx_bytes_) {}
  constexpr std::size_t bytes() const {
    return sizeof(double) * (std::size_t)ctx + ctx_bytes + kSlackBytes + sizeof(double) * (std::size_t)dl_doubles;
  }
};

// k_update_feat_stream<T> (viekf_kernels_stream.hpp)
struct UpdLds {
  int xs;      // [nxs]
  int W;       // [n][2]
  int K;       // [n][2]
  int lam;     // [n]
  int sm;      // [32] small scratch: zhat(2) Hb(4) res(2) Sinv(4) = 12, dxb(16)
  int total;
  constexpr UpdLds(int nxs, int n) : xs(0), W(nxs), K(W + 2 * n), lam(K + 2 * n), sm(lam + n), total(sm + 32) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

// k_update_generic<T> (viekf_kernels_generic.hpp)
struct GenLds {
  int xs;      // [nxs]
  int W;       // [n][3]
  int K;       // [n][3]
  int lam;     // [n]
  int sm;      // [64]: hcols (int as double) [0..5], Hc [6..23] (3 rows x 6 cols), res [24..26], ncol [27], Si [28..36], verdict [37]
  int total;
  constexpr GenLds(int nxs, int n) : xs(0), W(nxs), K(W + 3 * n), lam(K + 3 * n), sm(lam + n), total(sm + 64) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

// k_eval_xdot<T> (viekf_kernels_hooks.hpp)
struct XdotLds {
  static constexpr int kSlackBytes = 16;   // (as PropLds)
  int xs;      // [nxs]
  int Abb;     // 16x16 row-major
  int Gb;      // 16x6
  int xdb;     // 16
  int ctx;     // BodyCtx, ctx_bytes bytes
  std::size_t ctx_bytes;
  constexpr XdotLds(int nxs, std::size_t ctx_bytes_) : xs(0), Abb(nxs), Gb(Abb + 256), xdb(Gb + 96), ctx(xdb + 16), ctx_bytes(ctx_bytes_) {}
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)ctx + ctx_bytes + kSlackBytes; }
};

// k_keep_features<T> (viekf_kernels_lifecycle.hpp): doubles and ints share the buffer, so these offsets are in BYTES
struct KeepLds {
  std::size_t colbuf;   // double [n]  the column in flight
  std::size_t srcrow;   // int [n]     old row index of new row i (or -1)
  std::size_t cnt;      // int [4]     the number of features kept (+ 3 spare)
  std::size_t total;
  constexpr explicit KeepLds(int n)
      : colbuf(0), srcrow(sizeof(double) * (std::size_t)n), cnt(srcrow + sizeof(int) * (std::size_t)n), total(cnt + sizeof(int) * 4) {}
  constexpr std::size_t bytes() const { return total; }
};

}  // namespace viekf
