// viekf_instance_rows.hpp -- THE list of fused-step kernel instances: one X-macro row per instance, written here and nowhere
// else.  The explicit instantiations (viekf_inst.hip), their `extern template` declarations and the index -> kernel tables
// (both viekf_dispatch.hpp) and the dispatch rows below all expand these lists.  No HIP here: viekf_resmap.cpp includes it too.
#pragma once

// Resident family, X(RB, NW, NS, nmin, nmax, max_lds_kb): NW worker waves + NS service waves per workgroup (NS = 2: the body
// lanes on a wave of their own), feature counts nmin .. nmax.  Symmetric ownership: the N (N + 1) / 2 owned 3x3 blocks are dealt
// to the NW * 64 worker threads by build_resmap (viekf_resmap.cpp), at most RB per thread.  The first row that holds a batch
// wins, and the row ORDER is the VIEKF_TUNE_RES_INSTANCE index: rows are appended or dropped, never reordered.  The _g lists are
// the groups viekf_inst.hip compiles in parallel.
//  <2, 1>  the reference's own sizes (NUM_FEATURES 12, params 20 -> here up to 15): ONE worker wave + the service wave, four
//          128-thread workgroups per CU (LDS <= 40 KB) -- a small filter's step is its update chain's latency, so the CU is
//          filled with chains
#define VIEKF_RES_LIST_0(X) X(2, 1, 1, 1, 15, 40) X(2, 2, 1, 1, 22, 80)
//  <3, 2>  small filters: 192-thread workgroups, two per CU (LDS <= 80 KB, <= 256 VGPRs): one filter's update chain runs under
//          the other's sweeps
//  <4, 3>  (a 7-slot instance sweeps 7 slots per update however few the map fills: N = 32 needs 3)
#define VIEKF_RES_LIST_1(X) X(3, 2, 1, 1, 25, 80) X(4, 3, 1, 26, 38, 80)
#define VIEKF_RES_LIST_2(X) X(5, 3, 1, 39, 43, 80) X(6, 3, 1, 44, 47, 80)
//  <7, 3>  two 256-thread workgroups per CU at the headline size (7 blocks per thread, LDS <= 80 KB)
//  <1, 7>  one workgroup per CU (small batches): again the smallest instance that holds the size
#define VIEKF_RES_LIST_3(X) X(7, 3, 1, 26, 50, 80) X(1, 7, 1, 1, 29, 160)
#define VIEKF_RES_LIST_4(X) X(2, 7, 1, 30, 41, 160) X(3, 7, 1, 1, 50, 160)
//  <5, 6>  more features than one service wave has lanes for (N + 14 > 64): two service waves
//  <6, 6>  ... and, past 64, features 64.. on the body wave's free lanes
#define VIEKF_RES_LIST_5(X) X(5, 6, 2, 51, 57, 160) X(6, 6, 2, 51, 67, 160)
//  <8, 6>  8 blocks per thread: the register file's end (3 scratch operations per update in the worker loop)
#define VIEKF_RES_LIST_6(X) X(7, 6, 2, 65, 72, 160) X(8, 6, 2, 73, 77, 160)
// (<4, 5> -- two 384-thread workgroups per CU, three waves per SIMD at <= 168 VGPRs -- measured 32 % slower: dropped)
// (<4, 6> -- 4 blocks per thread on 6 worker waves, the service wave alone on its SIMD -- measured 4 % slower: dropped)
#define VIEKF_RES_LIST(X) \
  VIEKF_RES_LIST_0(X) VIEKF_RES_LIST_1(X) VIEKF_RES_LIST_2(X) VIEKF_RES_LIST_3(X) VIEKF_RES_LIST_4(X) VIEKF_RES_LIST_5(X) VIEKF_RES_LIST_6(X)

// Tile family, X(NT, NW, pair_lds_kb, single_lds_kb): NT tiles per side (an instance runs the feature counts with
// 1 + ceil(N / 5) == NT: its tile -> wave map is compile-time), NW worker waves + 1 service wave (N + 14 <= 64 lanes).  Every
// row is TWO dispatch rows, in this order: the pair form -- TWO filters per 512-thread workgroup, one workgroup per CU, their
// update loops half a phase out of step (k_step_tiles_pair), the form for batches beyond one filter per CU -- and the single
// form, one filter per 256-thread workgroup.
//  <11, 3>  N = 46 .. 50: the headline instance
#define VIEKF_TILE_LIST_7(X) X(11, 3, 160, 80)
#define VIEKF_TILE_LIST(X) VIEKF_TILE_LIST_7(X)
#define VIEKF_INST_GROUPS 8

namespace viekf {

struct ResInst { int RB, NW, NS, nmin, nmax, max_lds_kb; };
struct TileInst { int NT, NW, max_lds_kb, pair; };

// The PACKED image of P: between two fused launches a filter's n * ld doubles of the P buffer may hold the
// kernel's own register and LDS image instead of the column-major matrix -- offsets in doubles from the filter's P:
//   [0, single)       the worker threads' blocks: register q = 9 * slot + element of thread t, in pairs (q, q + 1) of 16
//                     bytes per lane, pair p of the TW = 64 NW threads contiguous: offset 2 (p TW + t) + (q & 1)
//   [single, pbc)     the last register of an odd count (9 RB odd), 8 bytes per lane: offset single + t
//   [pbc, pbb)        the body columns as they sit in LDS, Pbc[3N][16];   [pbb, total)  the body block Pbb[16][16]
// The map (thread, slot) -> block is build_resmap's, so an image is defined by (instance row, N).  THE FIT RULE: the packed
// form is used only where `total` <= n * ld (fits); a small N on a wide instance does not fit and stays canonical.
struct ResPack {
  int TW, npair, single, pbc, pbb, total;
  constexpr ResPack(int N, int RB, int NW)
      : TW(64 * NW), npair(9 * RB / 2), single(2 * (9 * RB / 2) * 64 * NW), pbc(single + ((9 * RB) & 1) * 64 * NW),
        pbb(pbc + 48 * N), total(pbc + 48 * N + 256) {}
  constexpr int elem(int q, int t) const { return q < 2 * npair ? 2 * ((q >> 1) * TW + t) + (q & 1) : single + t; }
  // element (r, c), r >= c, of the body block P[0..16, 0..16]: Pbb is row-major, and its entry [r][c] is what an unpack stores
  // at row r of column c (viekf_node_global reads its 21 elements through this, viekf_capi.hip)
  constexpr int body(int r, int c) const { return pbb + 16 * r + c; }
  constexpr bool fits(int n, int ld) const { return (long)total <= (long)n * ld; }
};

#define VIEKF_RES_ROW(RB, NW, NS, NMIN, NMAX, KB) {RB, NW, NS, NMIN, NMAX, KB},
#define VIEKF_TILE_ROWS(NT, NW, PAIR_KB, SINGLE_KB) {NT, NW, PAIR_KB, 1}, {NT, NW, SINGLE_KB, 0},
inline constexpr ResInst kResInst[] = {VIEKF_RES_LIST(VIEKF_RES_ROW)};
inline constexpr TileInst kTileInst[] = {VIEKF_TILE_LIST(VIEKF_TILE_ROWS)};
#undef VIEKF_RES_ROW
#undef VIEKF_TILE_ROWS
constexpr int kNumResInst = (int)(sizeof(kResInst) / sizeof(kResInst[0]));
constexpr int kNumTileInst = (int)(sizeof(kTileInst) / sizeof(kTileInst[0]));

}  // namespace viekf
