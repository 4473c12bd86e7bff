// viekf_fused_lds.hpp -- the fused step's LDS, written ONCE for host and device: the carve-ups of the resident and the tile
// family (ResLds, TileLds: the kernel takes its pointers from the struct, the launch its byte count), the word map of the
// scratchpad `sm` through which the waves of a workgroup talk to each other, and the launch word of the fused kernels.
// Plain C++17, no HIP header: a host compiler includes it too (tests/cpp/fused_lds_model.cpp checks every layout for every N,
// the word maps and the launch word).  Offsets are in doubles from the start of the (filter's) dynamic LDS.
// sizeof(BodyCtx) cannot be seen from here: the caller passes it in (ctx_bytes).
#pragma once
#include <cstddef>

#include "viekf_instance_rows.hpp"

#if defined(__HIPCC__)
#define VIEKF_HD __host__ __device__
#else
#define VIEKF_HD
#endif

namespace viekf {

// ---- the launch word ------------------------------------------------------------------------------------------------------
// The second argument of every fused kernel (`do_prop`), uniform over the launch:
//   bit 0       propagate          bits 1..3   RES_FMT_* (the resident family reads them)
//   bits 8..15  timing-only ablation bits of a -DVIEKF_ABLATE build (else 0)
//   bits 16..   KP, the propagates of the launch -- travels with the propagate bit only; 0 reads as 1
// Format bits: which form of P the launch loads and which it stores -- canonical column-major P[n][ld] (lower triangle valid) or
// the packed image of the kernel's own registers and LDS (ResPack, viekf_instance_rows.hpp) -- and the conversion-only launch (no
// propagate, M = 0): it leaves x, the status words and the result buffers alone, so packed -> canonical is an identity on
// everything but the form.
constexpr int RES_FMT_LOAD_PACKED = 1, RES_FMT_STORE_PACKED = 2, RES_FMT_P_ONLY = 4;
constexpr int launch_pack(bool prop, int kp, int fmt, int dbg) { return (prop ? (1 | (kp << 16)) : 0) | (fmt << 1) | ((dbg & 0xff) << 8); }
constexpr int launch_prop(int w) { return w & 1; }
constexpr int launch_fmt(int w) { return (w >> 1) & 7; }
constexpr int launch_dbg(int w) { return (w >> 8) & 0xff; }
constexpr int launch_kp(int w) { return (w >> 16) > 0 ? (w >> 16) : 1; }

// ---- the scratchpad's word map --------------------------------------------------------------------------------------------
// A row per group of words.  `zero`: the prologue clears it (every word that must read zero when the step starts, and word 49 of
// the resident family, which it has always cleared); `live`: the configurations in which somebody READS it -- a word that is live
// nowhere is dead.
enum : unsigned { SM_RES1 = 1, SM_RES2 = 2, SM_TILE = 4, SM_TILE_PAIR = 8 };   // one / two service waves; tile single / pair
struct SmWords {
  const char* name;
  int at, count;        // words [at, at + count)
  bool is_int;          // an int in a double's slot (else a double)
  bool zero;
  unsigned live;
  const char* writer;
  const char* reader;
};

// Resident family (k_step_resident).  par: parity of the fix_depth mailbox, phase: the update's count `cnt`, mb: mailbox 0 / 1,
// role: 0 the one service wave, 1 / 2 the feature / body wave of two (res_service).  Words 34..35, 38..39, 43, 47..48, 55..63 are
// reserved.  The prologue clears the same words in every instance -- the second service wave's also where there is none, and dead
// word 49: without those eight stores the code behind them shifts by a few bytes, and single instances' step times moved by up to
// 2 % either way (profiles/fused_lds/README.md).
namespace res_sm {
// the hand-over of a measurement's uniform values between two service waves: mailbox mb is words [16 mb, 16 mb + MB_FIELDS)
enum { MB_H0, MB_H1, MB_H2, MB_H3, MB_R0, MB_R1, MB_S0, MB_S1, MB_S2, MB_S3, MB_GATE, MB_FIELDS };
constexpr int MB_STRIDE = 16;
constexpr int mbox(int mb) { return MB_STRIDE * mb; }
constexpr int mbox_seq(int mb) { return 32 + mb; }                               // int: sequence number of mailbox mb
constexpr int fix_word(int role, int par) { return (role == 2 ? 36 : 40) + par; }     // "fix mailbox non-empty", one word per service wave
constexpr int DT = 42;
constexpr int nan_word(int role, int phase) { return (role == 2 ? 52 : 44) + phase % 3; }   // NaN-guard word, one per service wave
constexpr int gate_word(int phase) { return 50 + (phase & 1); }                       // gate verdict
constexpr int CTRL_WORDS = 64;                                                   // the words above and their reserved neighbours
constexpr int SQRTQU = CTRL_WORDS, QXB = SQRTQU + 6;   // launch constants the propagate reads inside its barrier intervals: at fixed
                                                       // offsets from sm they cost no pointer of their own (staged instances only)
constexpr int len(bool staged) { return staged ? QXB + 16 : CTRL_WORDS; }
inline constexpr SmWords kWords[] = {
    {"mailbox 0", mbox(0), MB_FIELDS, false, false, SM_RES2, "the service wave that holds the feature (send)", "the other service wave (recv)"},
    {"mailbox 1", mbox(1), MB_FIELDS, false, false, SM_RES2, "the service wave that holds the feature (send)", "the other service wave (recv)"},
    {"mailbox sequence numbers", mbox_seq(0), 2, true, true, SM_RES2, "send", "recv (polls)"},
    {"fix mailbox non-empty, body wave", fix_word(2, 0), 2, false, true, SM_RES2, "service role 2", "workers (fix_word)"},
    {"fix mailbox non-empty", fix_word(0, 0), 2, false, true, SM_RES1 | SM_RES2, "service role 0 / 1", "workers (fix_word)"},
    {"dt", DT, 1, false, false, SM_RES1 | SM_RES2, "prologue; service (next propagate of several)", "service, res_prop_setup"},
    {"NaN guard", nan_word(0, 0), 3, false, true, SM_RES1 | SM_RES2, "service role 0 / 1 (gain_rows)", "workers; service role 2"},
    {"(dead: once the count of published raw columns)", 49, 1, true, true, 0, "nobody", "nobody"},
    {"gate verdict", gate_word(0), 2, false, true, SM_RES1 | SM_RES2, "service role 0 / 1 (gain_rows)", "workers"},
    {"NaN guard, body wave", nan_word(2, 0), 3, false, true, SM_RES2, "service role 2 (gain_rows)", "workers; service role 1"},
    {"sqrt(Qu)", SQRTQU, 6, false, false, SM_RES1 | SM_RES2, "prologue", "res_prop_setup"},
    {"Qx of the body rows", QXB, 16, false, false, SM_RES1 | SM_RES2, "prologue", "res_prop_body"},
};
}  // namespace res_sm

// Tile family (k_step_tiles, k_step_tiles_pair): one service wave.  Its prologue clears the whole scratchpad, which covers the
// words marked zero.
namespace tile_sm {
enum { MB_G00, MB_G01, MB_G11, MB_SKIP, MB_FIELDS };   // mailbox mb is words [8 mb, 8 mb + MB_FIELDS)
constexpr int MB_STRIDE = 8;
constexpr int mbox(int mb) { return MB_STRIDE * mb; }
constexpr int fix_word(int par) { return 40 + par; }
constexpr int DT = 42;
constexpr int nan_word(int phase) { return 44 + phase % 3; }
constexpr int TRIPS = 60;                              // the number of updates that will run
constexpr int CTRL_WORDS = 64;
constexpr int len() { return CTRL_WORDS; }
inline constexpr SmWords kWords[] = {
    {"mailbox 0", mbox(0), MB_FIELDS, false, false, SM_TILE | SM_TILE_PAIR, "service (publish)", "workers"},
    {"mailbox 1", mbox(1), MB_FIELDS, false, false, SM_TILE | SM_TILE_PAIR, "service (publish)", "workers"},
    {"fix mailbox non-empty", fix_word(0), 2, false, true, SM_TILE | SM_TILE_PAIR, "service", "workers"},
    {"dt", DT, 1, false, false, SM_TILE | SM_TILE_PAIR, "prologue; service (next propagate of several)", "service, res_prop_setup"},
    {"NaN in the column pair", nan_word(0), 3, false, true, SM_TILE | SM_TILE_PAIR, "workers (set; clear two phases ahead)", "workers, service"},
    {"updates that will run", TRIPS, 1, false, false, SM_TILE_PAIR, "prologue", "both halves of a paired workgroup"},
};
}  // namespace tile_sm

// The words of the control block the prologue clears, bit w = word w: those marked zero.
template <int NWD>
constexpr unsigned long long sm_zero_mask(const SmWords (&words)[NWD]) {
  unsigned long long m = 0;
  for (int i = 0; i < NWD; i++)
    if (words[i].zero)
      for (int w = words[i].at; w < words[i].at + words[i].count; w++) m |= 1ull << w;
  return m;
}

// ---- the carve-ups --------------------------------------------------------------------------------------------------------
constexpr std::size_t kBodyCtxBytes = 440;   // sizeof(BodyCtx) as the model check takes it (viekf_dispatch.hpp asserts the real one)
// Propagate in low-rank coupling form.  A_fb[I] = Afv_I E_v + Afg_I E_g and the bias rows of A_bb are zero
// (vi_ekf_dyn.cpp:55-71,121-128), so  Phi_fb[I] = D_I Psi  with a per-feature 3x9  D_I = [M1 | M3 | M2],
//   M1 = (Afv + dt/2 Aff Afv) dt,  M3 = Afv dt^2/2,  M2 = (Afg + dt/2 Aff Afg) dt,   Psi = [E_v ; A_bb[vel rows] ; E_g]  (9 x 16),
// and with  Pi = Psi P_bb Psi^T,  V_I = Phi_ff[I] P[I, body],  Ut_I = D_I Pi / 2 + V_I Psi^T  (3x9):
//   P+[I,J] = Phi_ff[I] P[I,J] Phi_ff[J]^T + Ut_I D_J^T + D_I Ut_J^T + Gs_I Gs_J^T (+ Qx),   Gs = Gd sqrt(Qu)
//   P+[I,body] = V_I Phi_bb^T + D_I Xi + Gs_I Gs_b^T,   Xi = Psi (P_bb Phi_bb^T)
// -- a K = 24 contraction over ONE record per row (the symmetric form needs no separate X / Y operands):
//   Z[row] = { (Ut[k], D[k]) k = 0..8 interleaved | Gs[0..5] | pad }      ZS doubles per row
constexpr int ZK = 9;    // rank of the feature/body coupling
constexpr int ZS = 26;   // row stride of Z: 6 ZS = 28 (mod 64 dwords), consecutive features land on distinct 16-byte bank groups

// measurements per launch (the host chunks longer lists: P then makes one more HBM round trip per chunk): a frame that measures
// every feature once fits one launch.  (64 up to 64 features: the headline instance, <7, 3> at N = 50, takes 81 488 of its
// 81 920 bytes of LDS -- 432 are left.)
VIEKF_HD inline int res_mcap(int N) { return N > 64 ? 80 : 64; }

// Which instances batch their block loads, and stage sqrt(Qu) / Qx in LDS: all but the one-workgroup-per-CU instances <1,7>, <2,7>,
// <3,7> -- 1 to 3 blocks per thread leave next to nothing to batch, and their unit-Lambda step measured 0.7 - 1.4 % SLOWER with the
// batches -- and <8,6> at the register file's end (its propagate-only launch +1.8 %, more spilled dwords).  Those compile to the
// instruction stream they had before (profiles/serial_loads/).
constexpr bool res_batched_loads(int RB, int NW) { return NW != 7 && RB != 8; }

// Which kernels publish a feature's column pair with ONE store body per wave (extract_cols, res_worker).  build_resmap's lane pass
// leaves no worker thread with two blocks of a common feature (N = 50 on <7,3>: one thread with one such pair), so the lanes of a
// wave's slots that hold the published feature are disjoint: each moves its six oriented values and its row base into one set of
// temporaries, and three 16-byte stores behind the slot loop serve them all -- where every matching (slot, wave) group ran three
// stores of its own, each taking the VGPR -> LDS store path for about 13 cycles whether one lane is enabled or sixty-four.  A lane's
// second match stores from its slot as before, behind a branch a wave without such a lane skips.  The same values reach the same
// addresses, so results are bit for bit those of the per-slot form.  The gate covers the single-propagate kernels of <7,3>, the
// instance this was measured on; the multi-propagate kernels keep the per-slot statements and serve as the bit-for-bit reference.
// VIEKF_MERGED_PUBLISH=0 at build time restores every kernel, and a kernel whose gate is off compiles to the instruction stream it
// had before.
#ifndef VIEKF_MERGED_PUBLISH
#define VIEKF_MERGED_PUBLISH 1
#endif
constexpr bool res_merged_publish(int RB, int NW, bool MP) { return (VIEKF_MERGED_PUBLISH) != 0 && !MP && RB == 7 && NW == 3; }

struct ResLds {  // resident family; staged: res_batched_loads of the instance.  The words of sm: res_sm above
  int xs, Kt, Wt, Praw, lam, sm, fixadd, fixset, Z, phiff, Abb, Gb, Phibb, Mbb, Gdb, Pbb, T16, xdb, ctx, Pbc, PhibbT, Pd, PsiP, Pi, Xi, AvG, Lbc, mslot, mseq, mz, mR, img_len, total;
  VIEKF_HD ResLds(int N, int n, int nxs, bool staged, std::size_t ctx_bytes) {
    const int nf = 3 * N;
    int o = 0;
    auto take = [&](int cnt) { int r = o; o += (cnt + 1) & ~1; return r; };
    xs = take(nxs);
    lam = take(n);
    sm = take(res_sm::len(staged));
    fixadd = take(2 * (N > 0 ? N : 1)); fixset = take(2 * (N > 0 ? N : 1));
    // Z, Phi_ff and the two-lives region are contiguous: at store time all of it is dead and holds the P image
    Z = take(nf * ZS > 4 * n ? nf * ZS : 4 * n);   // propagate: the records; updates: second gain-row buffer; store: P image
    phiff = take(9 * (N > 0 ? N : 1));
    // one region, two lives: the propagate's body-sized scratch | the update loop's gain rows, raw columns and zeta blocks
    const int u0 = o;
    Abb = take(256); Gb = take(96); Phibb = take(256); PhibbT = take(256); Gdb = take(96); T16 = take(256);
    PsiP = take(ZK * 16); Pi = take(ZK * ZK); Xi = take(ZK * 16); AvG = take(18);
    const int uprop = o;
    o = u0;
    Kt = take(2 * n); Wt = take(2 * n);
    Praw = take(4 * n > 256 ? 4 * n : 256);   // two buffers [n][2]: raw column pairs of the next two measurements
    Pd = take(4 * (N > 0 ? N : 1));           // zeta-zeta 2x2 diagonal blocks, handed from the workers to the service lanes
    if (uprop > o) o = uprop;
    img_len = o - Z;
    Mbb = take(256); Pbb = take(256);
    xdb = take(16);
    ctx = take((int)((ctx_bytes + 7) / 8));
    Pbc = take(nf * 16);
    Lbc = take(48);   // Lambda of (feature row q, body column k): [3][16]
    const int mc = res_mcap(N);   // measurements per launch
    mslot = take(mc / 2); mseq = take(mc); mz = take(2 * mc); mR = take(4 * mc);
    total = o;
  }
};

VIEKF_HD inline int tile_nt(int N) { return 1 + (N + 4) / 5; }

struct TileLds {  // tile family.  The words of sm: tile_sm above
  int xs, lam, sm, fixadd, fixset, Z, phiff, Abb, Gb, Phibb, PhibbT, Gdb, T16, PsiP, Pi, Xi, AvG, Cb, Eb, Pd, Mbb, Pbb, xdb, ctx, Pbc,
      mslot, mseq, mz, mR, total;
  VIEKF_HD TileLds(int N, int n, int nxs, std::size_t ctx_bytes) {
    const int nf = 3 * N, NQ = 16 * tile_nt(N);
    int o = 0;
    auto take = [&](int cnt) { int r = o; o += (cnt + 1) & ~1; return r; };
    xs = take(nxs);
    lam = take(n);
    sm = take(tile_sm::len());
    fixadd = take(2 * (N > 0 ? N : 1)); fixset = take(2 * (N > 0 ? N : 1));
    Z = take(nf * ZS);      // the propagate's records
    phiff = take(9 * (N > 0 ? N : 1));
    // one region, two lives: the propagate's body-sized scratch | the update loop's column buffers
    const int u0 = o;
    Abb = take(256); Gb = take(96); Phibb = take(256); PhibbT = take(256); Gdb = take(96); T16 = take(256);
    PsiP = take(ZK * 16); Pi = take(ZK * ZK); Xi = take(ZK * 16); AvG = take(18);
    const int uprop = o;
    o = u0;
    Cb = take(4 * NQ);      // two buffers [NQ][2]: the column pair of the CURRENT measurement's feature, every pending update applied
    Eb = take(4 * NQ);      // two buffers [NQ][2]: raw column pairs extracted from the tiles one update ahead
    Pd = take(4 * (N > 0 ? N : 1));   // zeta-zeta 2x2 diagonal blocks, handed from the workers to the service lanes
    if (uprop > o) o = uprop;
    Mbb = take(256); Pbb = take(256);
    xdb = take(16);
    ctx = take((int)((ctx_bytes + 7) / 8));
    Pbc = take(nf * 16);    // the body columns P[16.., 0:16] during load and propagate (register tiles during the updates)
    const int mc = res_mcap(N);
    mslot = take(mc / 2); mseq = take(mc); mz = take(2 * mc); mR = take(4 * mc);
    total = o;
  }
  // word w of the scratchpad of filter `half` of a paired workgroup (its two carve-ups lie back to back), from the workgroup's LDS
  VIEKF_HD int pair_word(int half, int w) const { return half * total + sm + w; }
};

}  // namespace viekf
