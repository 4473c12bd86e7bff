// viekf_stream_lds.hpp -- the dynamic-LDS carve-ups of the streaming-side kernels, each written ONCE: the kernel takes its
// pointers from the struct, the launch site its byte count (bytes()), so the two cannot drift apart.  Plain C++17, no HIP header:
// a host compiler includes it too (tests/cpp/stream_lds_model.cpp checks every struct for every N).  Offsets are in doubles
// from the start of the dynamic LDS unless a struct says otherwise; the size of each region stands beside its offset.
// sizeof(BodyCtx) cannot be seen from here: the caller passes it in (ctx_bytes).
// At the end: the layouts of the wide-P path (WideLds, BlkLds, PsvLds) and grouped_choice, THE rule by which a batch gets one
// of the two grouped update kernels, with the LDS budget it is held to.
#pragma once
#include <cstddef>

#include "viekf_fused_lds.hpp"   // ZK, ZS: the propagate's record form

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

// ---- the wide-P path (P in HBM) ---------------------------------------------------------------------------------------------
// These three are carved by a running offset `o`: every region starts on an even double (16 bytes).
struct LdsTake {
  int total = 0;
  static constexpr int take(int& o, int doubles) { const int at = o; o += (doubles + 1) & ~1; return at; }
  constexpr std::size_t bytes() const { return sizeof(double) * (std::size_t)total; }
};

// k_propagate_wide<T> (viekf_kernels_wide.hpp)
struct WideLds : LdsTake {
  int xs = 0;       // [nxs]
  int Abb = 0;      // 16x16 row-major
  int Gb = 0;       // 16x6
  int Phibb = 0;    // 16x16
  int PhibbT = 0;   // 16x16, the transpose
  int Mbb = 0;      // 16x16
  int Gdb = 0;      // 16x6
  int Pbb = 0;      // 16x16 row-major copy of P_bb
  int T16 = 0;      // 16x16 scratch
  int xdb = 0;      // 16
  int ctx = 0;      // BodyCtx, ctx_bytes bytes
  int AvG = 0;      // 3x6
  int PsiP = 0;     // [ZK][16]
  int Pi = 0;       // [ZK][ZK]
  int Xi = 0;       // [ZK][16]
  int phiff = 0;    // [N][9] Phi_ff blocks
  int Z = 0;        // [3 N][ZS] the records
  int sm = 0;       // [8] spare
  constexpr WideLds(int N, int nxs, std::size_t ctx_bytes) {
    int o = 0;
    xs = take(o, nxs); Abb = take(o, 256); Gb = take(o, 96); Phibb = take(o, 256); PhibbT = take(o, 256); Mbb = take(o, 256);
    Gdb = take(o, 96); Pbb = take(o, 256); T16 = take(o, 256); xdb = take(o, 16); ctx = take(o, (int)((ctx_bytes + 7) / 8));
    AvG = take(o, 18); PsiP = take(o, ZK * 16); Pi = take(o, ZK * ZK); Xi = take(o, ZK * 16); phiff = take(o, 9 * N);
    Z = take(o, 3 * N * ZS); sm = take(o, 8);
    total = o;
  }
};

// What the two grouped feature updates (viekf_kernels_grouped.hpp) share: state, lambda, the panel and the S^-1 columns in front;
// the rho-rho diagonal, the slots of a group and a staged window of the measurement list behind what each kernel adds.  BG =
// measurements per group.  The int regions (gsl, gml, wsl and the kernels' own) start on doubles too: offsets in doubles as well.
struct GroupLds : LdsTake {
  int BLD = 0;      // row stride of the panel: 2 BG + 2 doubles (the MFMA operand reads, 16 consecutive rows, spread over the banks)
  int BWIN = 0;     // entries of a staged window: 2 BG
  int xs = 0;       // [nxs]
  int lam = 0;      // [n]
  int Wp = 0;       // [n rounded up to 16][BLD] the panel: raw zeta columns, turned into W rows
  int Si = 0;       // [BG][4] the two COLUMNS of S^-1 per measurement
  int diag = 0;     // [max(N, 1)] running P(rho_f, rho_f)
  int gsl = 0;      // int [BG] the group's slots                          } per group parity: the next one slot_stride doubles on
  int gml = 0;      // int [BG] their entries' indices into the window     }
  int slot_stride = 0;
  int wz = 0;       // [BWIN][2] pixels                                     } a window; per group parity: the next one win_stride
  int wR = 0;       // [BWIN][4] R, column-major 2x2                        } doubles on
  int wsl = 0;      // int [BWIN] the slot of an admitted entry, else -1    }
  int win_stride = 0;

 protected:
  constexpr void front(int& o, int n, int nxs, int BG) {
    BLD = 2 * BG + 2; BWIN = 2 * BG;
    xs = take(o, nxs); lam = take(o, n); Wp = take(o, ((n + 15) & ~15) * BLD); Si = take(o, 4 * BG);
  }
  // parities: 1 or 2 sets of slots and windows; slot_doubles: the doubles reserved per set of slots
  constexpr void back(int& o, int N, int BG, int parities, int slot_doubles) {
    diag = take(o, N > 0 ? N : 1);
    gsl = take(o, parities * slot_doubles); gml = gsl + BG / 2; slot_stride = slot_doubles;   // (BG is even)
    win_stride = 7 * BWIN;
    wz = take(o, parities * win_stride); wR = wz + 2 * BWIN; wsl = wR + 4 * BWIN;
    total = o;
  }
};

// k_update_feat_blocked<T, BG>
struct BlkLds : GroupLds {
  int pzz = 0;      // [2][4] zeta-zeta block of the current / next measurement     } in 32 doubles, the rest of them spare
  int badf = 0;     // int [BG] NaN-guard verdict of each measurement of the group  }
  constexpr BlkLds(int N, int n, int nxs, int BG) {
    int o = 0;
    front(o, n, nxs, BG);
    pzz = take(o, 32); badf = pzz + 8;
    back(o, N, BG, 1, 2 * BG);   // (twice the slots' room: the launch has always asked for it)
  }
};

// k_update_feat_panelsvc<T, BG>.  mail, ctab, cbuf, the slots and the window exist twice (group parity).
struct PsvLds : GroupLds {
  int mail = 0;     // [2][BG][12] per measurement {Hb[4], S^-1[4], r[2], gate, -}: service wave -> everybody
  int ctab = 0;     // [2][BG (BG - 1) / 2][4] per pair g < g': W_g of the two zeta rows of feature g' (the coupling of update g into pair g')
  int cbuf = 0;     // [2][BG][6] the group features' state {q_zeta[4], rho, P(rho, rho)} as the service wave leaves it: committed
                    // only when the speculation held
  int cpre = 0;     // [BG][6] the same BEFORE the group's own chain (through the previous group): what a failed speculation
                    // falls back to -- nobody else applied the previous group to these features
  int spec = 0;     // int [2] per parity: a K came out NaN (the speculation failed)
  int ticket = 0;   // int [1] the pass's unit counter (+ 1 spare int)
  int mail_sz = 0, ctab_sz = 0, cbuf_sz = 0;   // doubles per parity
  constexpr PsvLds(int N, int n, int nxs, int BG) {
    int o = 0;
    front(o, n, nxs, BG);
    mail_sz = 12 * BG; ctab_sz = 4 * BG * (BG - 1) / 2; cbuf_sz = 6 * BG;
    mail = take(o, 2 * mail_sz); ctab = take(o, 2 * ctab_sz); cbuf = take(o, 2 * cbuf_sz); cpre = take(o, cbuf_sz);
    spec = take(o, 2); ticket = spec + 1;
    back(o, N, BG, 2, BG);
  }
};

// ---- which grouped update a batch gets ----------------------------------------------------------------------------------------
// The look-ahead form (k_update_feat_panelsvc): groups of 16 -- the 48 rows of a group's features fit the serving wave -- where its
// double-buffered layout fits next to the panel (N <= 154).  Else k_update_feat_blocked with the forced group size, or the largest
// of 32 / 24 / 16 whose panel fits (fewer passes over P for the narrower filters; measured: at N = 64 groups of 32 are SLOWER
// than 16 -- 1.96 vs 1.83 ms per step, the sequential panel phase grows with the group -- while N = 100 gains 4 % from 24: the
// wider groups only where the passes dominate, n > 256).  none: one pass per measurement (k_update_feat_stream).
// What the kernels take for granted of a choice is what tests/cpp/stream_lds_model.cpp holds every choice to: one panel row per
// thread and a thread past every feature (n <= kGroupedThreads, blocked: thread T - 1, panelsvc: thread T - 65 >= N), the three
// 64-bit slot masks (N <= 192), a group's 3 BG rows on one wave (panelsvc), the LDS budget.
constexpr int kGroupedThreads = 512;
constexpr std::size_t kLdsBudgetBytes = 160 * 1024, kStaticLdsBytes = 1024;   // (the kernels' small static LDS)
constexpr bool grouped_fits(std::size_t bytes) { return bytes + kStaticLdsBytes <= kLdsBudgetBytes; }

enum class GroupedKernel { none, blocked, panelsvc };
struct GroupedChoice {
  GroupedKernel kernel;
  int BG;              // measurements per group (0 with none)
  std::size_t bytes;   // dynamic LDS of the launch
};
// tune_*: VIEKF_TUNE_BLOCK_GROUP (0 automatic, 16, 24, 32), VIEKF_TUNE_PANEL_SERVICE (0 / 1), VIEKF_TUNE_STREAM_MFMA (0 off, 1, 2)
constexpr GroupedChoice grouped_choice(int N, int n, int nxs, int tune_block_group, int tune_panel_svc, int tune_stream_mfma) {
  if (tune_stream_mfma == 0 || n > kGroupedThreads) return {GroupedKernel::none, 0, 0};
  if (tune_panel_svc != 0 && (tune_block_group == 0 || tune_block_group == 16)) {
    const std::size_t bytes = PsvLds(N, n, nxs, 16).bytes();
    if (grouped_fits(bytes)) return {GroupedKernel::panelsvc, 16, bytes};
  }
  const int cands[4] = {tune_block_group, 32, 24, 16};   // (a forced size first, whatever n)
  for (int k = 0; k < 4; k++) {
    const int cand = cands[k];
    if (cand == 0 || (k > 0 && cand > 16 && n <= 256)) continue;
    const std::size_t bytes = BlkLds(N, n, nxs, cand).bytes();
    if (grouped_fits(bytes)) return {GroupedKernel::blocked, cand, bytes};
  }
  return {GroupedKernel::none, 0, 0};
}

}  // namespace viekf
