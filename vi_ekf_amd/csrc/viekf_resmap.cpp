// viekf_resmap.cpp -- the block ownership map of the fused-step kernel (k_step_resident): pure host arithmetic, no HIP.
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

#include "viekf_host.hpp"
#include "viekf_instance_rows.hpp"

// Ownership map of the fused-step kernel: which 3x3 feature block P[16+3I.., 16+3J..] (I >= J: one of each symmetric pair)
// lives in slot `a` of worker thread t.  Entry [a][t] = I | J << 8 | owned << 16.
//  * slot 0 of the threads t < N holds the diagonal blocks (t, t) (the kernel's own_diag convention);
//  * every other (slot, wave) pair is a GROUP of 64 lanes.  The strictly lower blocks are cut into 8 x 8 tiles of features;
//    a full tile fills one group with lane = 8 i + j  <->  block (8 TI + i, 8 TJ + j).  Every update publishes the column
//    pair of ONE feature s from the registers that hold it: the blocks {., s} then sit in the few groups whose tile row or
//    tile column contains s -- at N = 50 on three worker waves 2.6 groups per wave on average (at most 4) instead of 6.7
//    (at most 7) with the blocks dealt round-robin along wrapped diagonals (r01/r02a), and each group costs its wave the
//    whole extraction body whether one lane matches or eight.  The LDS reads of a tile's operand rows (K rows by i, W rows by
//    j: 48 bytes apart) are conflict-free in every 16-lane service group of ds_read_b128.
//  * what is left (the triangles of the diagonal tiles, the ragged last tile row when N is not a multiple of 8) is packed
//    unit by unit into the remaining lanes, best fit first.
// Returns false when the blocks do not fit RB slots of TW threads.
bool viekf::build_resmap(int N, int RB, int NWV, std::vector<int>& map, int* used_slots) {
  const int TW = 64 * NWV;
  map.assign((size_t)RB * TW, 0);
  if (N > TW || N > 255) return false;
  auto put = [&](int slot, int t, int I, int J) { map[(size_t)slot * TW + t] = I | (J << 8) | (1 << 16); };
  for (int t = 0; t < N; t++) put(0, t, t, t);
  struct Group { int slot, wave; std::vector<int> free_lanes; };
  std::vector<Group> groups;
  for (int s = 0; s < RB; s++)
    for (int w = 0; w < NWV; w++) {
      Group g{s, w, {}};
      for (int l = 0; l < 64; l++)
        if (!(s == 0 && 64 * w + l < N)) g.free_lanes.push_back(l);
      groups.push_back(g);
    }
  typedef std::vector<std::pair<int, int>> Unit;
  std::vector<Unit> ragged;
  const int kf = N / 8, r = N % 8;
  for (int TI = 0; TI < kf; TI++)
    for (int TJ = 0; TJ < TI; TJ++) {
      // a full group, preferably on wave (TI + TJ) mod NWV: the tiles of one tile row / column then spread over the waves
      const int pref = (TI + TJ) % NWV;
      int best = -1, bestkey = 1 << 30;
      for (int g = 0; g < (int)groups.size(); g++) {
        if (groups[g].free_lanes.size() != 64) continue;
        const int key = ((groups[g].wave - pref + NWV) % NWV) * 64 + groups[g].slot;
        if (key < bestkey) { bestkey = key; best = g; }
      }
      if (best < 0) {
        Unit u;
        for (int i = 0; i < 8; i++)
          for (int j = 0; j < 8; j++) u.push_back({8 * TI + i, 8 * TJ + j});
        ragged.push_back(u);
        continue;
      }
      for (int i = 0; i < 8; i++)
        for (int j = 0; j < 8; j++) put(groups[best].slot, 64 * groups[best].wave + 8 * i + j, 8 * TI + i, 8 * TJ + j);
      groups[best].free_lanes.clear();
    }
  for (int TD = 0; TD < kf; TD++) {
    Unit u;
    for (int i = 0; i < 8; i++)
      for (int j = 0; j < i; j++) u.push_back({8 * TD + i, 8 * TD + j});
    ragged.push_back(u);
  }
  if (r) {
    for (int TJ = 0; TJ < kf; TJ++) {
      Unit u;
      for (int i = 0; i < r; i++)
        for (int j = 0; j < 8; j++) u.push_back({8 * kf + i, 8 * TJ + j});
      ragged.push_back(u);
    }
    Unit u;
    for (int i = 0; i < r; i++)
      for (int j = 0; j < i; j++) u.push_back({8 * kf + i, 8 * kf + j});
    if (!u.empty()) ragged.push_back(u);
  }
  std::stable_sort(ragged.begin(), ragged.end(), [](const Unit& x, const Unit& y) { return x.size() > y.size(); });
  for (const Unit& u : ragged) {
    int best = -1;
    size_t bestslack = ~(size_t)0;
    for (int g = 0; g < (int)groups.size(); g++) {
      const size_t f = groups[g].free_lanes.size();
      if (f >= u.size() && f - u.size() < bestslack) { bestslack = f - u.size(); best = g; }
    }
    size_t k = 0;
    if (best >= 0) {
      Group& G = groups[best];
      for (; k < u.size(); k++) { put(G.slot, 64 * G.wave + G.free_lanes.front(), u[k].first, u[k].second); G.free_lanes.erase(G.free_lanes.begin()); }
      continue;
    }
    // no group takes the unit whole: split it over the emptiest ones
    while (k < u.size()) {
      int big = -1;
      for (int g = 0; g < (int)groups.size(); g++)
        if (!groups[g].free_lanes.empty() && (big < 0 || groups[g].free_lanes.size() > groups[big].free_lanes.size())) big = g;
      if (big < 0) return false;
      Group& G = groups[big];
      while (k < u.size() && !G.free_lanes.empty()) {
        put(G.slot, 64 * G.wave + G.free_lanes.front(), u[k].first, u[k].second);
        G.free_lanes.erase(G.free_lanes.begin());
        k++;
      }
    }
  }
  // Which WAVE a group sits on is still free (a wave sweeps all its slots alike): exchange whole groups between waves while
  // that lowers, in this order, the largest number of groups any wave has to publish from for one feature (the update's
  // waves meet at a barrier: the slowest one counts), the sum over the features of that maximum, and the sum of squares.
  // N = 50 on three waves: at most 4 -> 3 groups; N = 64 on six: 4 -> 2.
  if (N <= 128) {
    typedef unsigned __int128 fmask_t;
    const int ng = RB * NWV;
    std::vector<fmask_t> mask(ng, (fmask_t)0);   // features with a block in group (slot, wave) = index slot * NWV + wave
    auto remask = [&](int g) {
      fmask_t mk = 0;
      const int slot = g / NWV, wave = g % NWV;
      for (int l = 0; l < 64; l++) {
        const int e = map[(size_t)slot * TW + 64 * wave + l];
        if (e >> 16) mk |= ((fmask_t)1 << (e & 0xff)) | ((fmask_t)1 << ((e >> 8) & 0xff));
      }
      mask[g] = mk;
    };
    for (int g = 0; g < ng; g++) remask(g);
    struct Cost { long mx, summx, sq; bool operator<(const Cost& o) const { return mx != o.mx ? mx < o.mx : (summx != o.summx ? summx < o.summx : sq < o.sq); } };
    auto cost = [&]() {
      Cost c{0, 0, 0};
      for (int f = 0; f < N; f++) {
        long fm = 0;
        for (int w = 0; w < NWV; w++) {
          long cnt = 0;
          for (int sl = 0; sl < RB; sl++) cnt += (long)((mask[sl * NWV + w] >> f) & 1);
          fm = std::max(fm, cnt);
          c.sq += cnt * cnt;
        }
        c.mx = std::max(c.mx, fm);
        c.summx += fm;
      }
      return c;
    };
    auto whole = [&](int g) { return !(g / NWV == 0 && 64 * (g % NWV) < N); };   // (not sharing its lanes with the diagonal blocks)
    Cost best = cost();
    for (bool improved = true; improved;) {
      improved = false;
      for (int g1 = 0; g1 < ng; g1++)
        for (int g2 = g1 + 1; g2 < ng; g2++) {
          if (!whole(g1) || !whole(g2) || g1 % NWV == g2 % NWV) continue;
          std::swap(mask[g1], mask[g2]);
          const Cost c = cost();
          if (c < best) {
            best = c;
            improved = true;
            int* p1 = &map[(size_t)(g1 / NWV) * TW + 64 * (g1 % NWV)];
            int* p2 = &map[(size_t)(g2 / NWV) * TW + 64 * (g2 % NWV)];
            for (int l = 0; l < 64; l++) std::swap(p1[l], p2[l]);
          } else {
            std::swap(mask[g1], mask[g2]);
          }
        }
    }
  }
  // Which SLOT of its wave a group sits in is free as well: every wave's non-empty groups move to its lowest slots (slot 0
  // keeps the diagonal blocks), and the kernel's per-slot loops stop at the highest slot any wave uses -- a 7-slot instance
  // that holds N = 32 (3 slots' worth of blocks) then sweeps 3 slots per update, not 7.
  int used = 1;
  for (int w = 0; w < NWV; w++) {
    int dst = (64 * w < N) ? 1 : 0;   // (slot 0 of a wave that holds diagonal blocks stays where it is)
    for (int sl = dst; sl < RB; sl++) {
      bool any = false;
      for (int l = 0; l < 64 && !any; l++) any = (map[(size_t)sl * TW + 64 * w + l] >> 16) != 0;
      if (!any) continue;
      if (sl != dst)
        for (int l = 0; l < 64; l++) std::swap(map[(size_t)sl * TW + 64 * w + l], map[(size_t)dst * TW + 64 * w + l]);
      dst++;
    }
    used = std::max(used, dst);
  }
  if (used_slots) *used_slots = used;
  // Which LANE of its group a block sits in is free too (slot 0 of the threads t < N keeps the diagonal blocks): lanes are
  // permuted inside each (slot, wave) group until no worker thread holds two blocks with a common feature, or as few such
  // (thread, feature) repeats as the search reaches.  The lanes of a wave's slots that hold feature s are then disjoint, and
  // the wave publishes the column pair of s from all its slots with ONE store body (res_merged_publish).  Group by group, the
  // blocks of a group are re-assigned to its lanes at the least number of repeats against the thread's other slots (an
  // assignment problem of at most 64 x 64), and among those with the fewest blocks moved; rounds over a wave's groups repeat
  // while the count falls.  A full 8 x 8 tile stays conflict-free in its operand reads under any permutation of its lanes (its
  // 8 rows I and 8 columns J are consecutive features: 16-byte rows 3 apart, distinct modulo the 16 rows of the 64 banks).
  for (int w = 0; w < NWV; w++)
    for (int round = 0, before = resmap_wave_repeats(map, RB, NWV, w); before > 0 && round < 8; round++) {
      for (int sl = 0; sl < used; sl++) {
        std::vector<int> lanes;
        for (int l = 0; l < 64; l++)
          if (!(sl == 0 && 64 * w + l < N)) lanes.push_back(l);
        const int m = (int)lanes.size();
        if (m < 2) continue;
        // cnt[q][f]: how many OTHER slots of lane lanes[q] hold feature f
        std::vector<std::vector<unsigned char>> cnt(m, std::vector<unsigned char>(256, 0));
        for (int q = 0; q < m; q++)
          for (int s2 = 0; s2 < RB; s2++) {
            const int e = map[(size_t)s2 * TW + 64 * w + lanes[q]];
            if (s2 == sl || !(e >> 16)) continue;
            cnt[q][e & 0xff]++;
            if (((e >> 8) & 0xff) != (e & 0xff)) cnt[q][(e >> 8) & 0xff]++;
          }
        std::vector<int> ent(m);
        for (int p = 0; p < m; p++) ent[p] = map[(size_t)sl * TW + 64 * w + lanes[p]];
        std::vector<std::vector<long>> cost(m, std::vector<long>(m, 0));
        for (int p = 0; p < m; p++)
          for (int q = 0; q < m; q++) {
            long c = 0;
            if (ent[p] >> 16) c = (cnt[q][ent[p] & 0xff] ? 1 : 0) + (cnt[q][(ent[p] >> 8) & 0xff] ? 1 : 0);
            cost[p][q] = c * 1024 + (p != q ? 1 : 0);
          }
        const std::vector<int> to = resmap_assign(cost);
        for (int p = 0; p < m; p++) map[(size_t)sl * TW + 64 * w + lanes[to[p]]] = ent[p];
      }
      const int after = resmap_wave_repeats(map, RB, NWV, w);
      if (after >= before) break;
      before = after;
    }
  return true;
}

// (thread, feature) repeats of worker wave w: over its threads and the features, the blocks of the thread that hold the
// feature, less one
int viekf::resmap_wave_repeats(const std::vector<int>& map, int RB, int NWV, int w) {
  const int TW = 64 * NWV;
  int rep = 0;
  for (int l = 0; l < 64; l++) {
    int cnt[256] = {0};
    for (int sl = 0; sl < RB; sl++) {
      const int e = map[(size_t)sl * TW + 64 * w + l];
      if (!(e >> 16)) continue;
      const int I = e & 0xff, J = (e >> 8) & 0xff;
      if (cnt[I]++) rep++;
      if (J != I && cnt[J]++) rep++;
    }
  }
  return rep;
}

// Assignment problem: row p goes to column to[p], every column taken once, the sum of cost[p][to[p]] the least (the Hungarian
// method with potentials, O(m^3); deterministic)
std::vector<int> viekf::resmap_assign(const std::vector<std::vector<long>>& cost) {
  const int m = (int)cost.size();
  const long INF = 1L << 60;
  std::vector<long> u(m + 1, 0), v(m + 1, 0);
  std::vector<int> p(m + 1, 0), way(m + 1, 0);
  for (int i = 1; i <= m; i++) {
    p[0] = i;
    int j0 = 0;
    std::vector<long> minv(m + 1, INF);
    std::vector<char> usedc(m + 1, 0);
    do {
      usedc[j0] = 1;
      const int i0 = p[j0];
      long delta = INF;
      int j1 = 0;
      for (int j = 1; j <= m; j++) {
        if (usedc[j]) continue;
        const long cur = cost[i0 - 1][j - 1] - u[i0] - v[j];
        if (cur < minv[j]) { minv[j] = cur; way[j] = j0; }
        if (minv[j] < delta) { delta = minv[j]; j1 = j; }
      }
      for (int j = 0; j <= m; j++) {
        if (usedc[j]) { u[p[j]] += delta; v[j] -= delta; }
        else minv[j] -= delta;
      }
      j0 = j1;
    } while (p[j0] != 0);
    do {
      const int j1 = way[j0];
      p[j0] = p[j1];
      j0 = j1;
    } while (j0);
  }
  std::vector<int> to(m, 0);
  for (int j = 1; j <= m; j++) to[p[j] - 1] = j - 1;
  return to;
}

extern "C" {

// diagnostic hook (not part of include/viekf.h; host arithmetic only, no device needed): the fused-step kernel's block
// ownership map for n_feat features on `nw` worker waves with `rb` slots per thread -> out[rb * 64 * nw] entries
// I | J << 8 | owned << 16; -1 when the blocks do not fit.  tests/test_resmap_cpu.py checks its invariants.
int viekf_debug_build_resmap(int n_feat, int rb, int nw, int32_t* out) {   // returns the number of slots in use (> 0), -1 on failure
  std::vector<int> map;
  int used = 0;
  if (n_feat < 1 || rb < 1 || nw < 1 || !out) return -1;
  if (n_feat * (n_feat + 1) / 2 > rb * nw * 64 || !viekf::build_resmap(n_feat, rb, nw, map, &used)) return -1;
  for (size_t i = 0; i < map.size(); i++) out[i] = map[i];
  return used;
}

// diagnostic hook (not part of include/viekf.h; host arithmetic only): the (thread, feature) repeats the map's lane pass left,
// per worker wave -> out[nw]; returns their sum, -1 when the blocks do not fit.  tests/test_resmap_repeats_cpu.py recounts them.
int viekf_debug_resmap_repeats(int n_feat, int rb, int nw, int32_t* out) {
  std::vector<int> map;
  if (n_feat < 1 || rb < 1 || nw < 1 || !out) return -1;
  if (n_feat * (n_feat + 1) / 2 > rb * nw * 64 || !viekf::build_resmap(n_feat, rb, nw, map)) return -1;
  int sum = 0;
  for (int w = 0; w < nw; w++) sum += out[w] = viekf::resmap_wave_repeats(map, rb, nw, w);
  return sum;
}

// diagnostic hook (not part of include/viekf.h): row i of the resident dispatch table (viekf_instance_rows.hpp, the index
// VIEKF_TUNE_RES_INSTANCE takes); -1 past the end.  tests/test_resmap_cpu.py walks the table with it.
int viekf_debug_res_instance(int i, int* rb, int* nw, int* nmin, int* nmax) {
  if (i < 0 || i >= viekf::kNumResInst || !rb || !nw || !nmin || !nmax) return -1;
  const viekf::ResInst& r = viekf::kResInst[i];
  *rb = r.RB; *nw = r.NW; *nmin = r.nmin; *nmax = r.nmax;
  return 0;
}

// diagnostic hook (not part of include/viekf.h; host arithmetic only): the packed image of P (ResPack, viekf_instance_rows.hpp)
// of n_feat features on an instance with `rb` slots and `nw` worker waves.  elem[(9 * slot + element) * 64 nw + t] = offset, in
// doubles from the filter's P, of that register of worker thread t; info[0..4] = {offset of Pbc [3 n_feat][16], offset of Pbb
// [256], total, n * ld of the filter's P, fits (the host's rule)}.  tests/test_packed_layout_cpu.py checks its invariants.
int viekf_debug_packed_layout(int n_feat, int rb, int nw, int32_t* elem, int32_t* info) {
  if (n_feat < 1 || rb < 1 || nw < 1 || !elem || !info) return -1;
  const viekf::ResPack K(n_feat, rb, nw);
  for (int q = 0; q < 9 * rb; q++)
    for (int t = 0; t < K.TW; t++) elem[(size_t)q * K.TW + t] = K.elem(q, t);
  const int n = 16 + 3 * n_feat, ld = viekf::cov_ld(n_feat);
  info[0] = K.pbc; info[1] = K.pbb; info[2] = K.total; info[3] = n * ld; info[4] = K.fits(n, ld) ? 1 : 0;
  return 0;
}

}  // extern "C"
