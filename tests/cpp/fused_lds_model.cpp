// Model check of the fused step's LDS (vi_ekf_amd/csrc/viekf_fused_lds.hpp), stand-alone on a CPU: the header is plain C++17, this
// program includes nothing else of the library.    fused_lds_model tests/golden/fused_lds_totals.txt
//   (a) ResLds for N = 1 .. 77, both values of `staged`, and TileLds for N = 1 .. 50, each for several sizes of BodyCtx: every
//       region inside `total` and on a 16-byte boundary, regions of one life pairwise disjoint, the two lives of the shared region
//       start together and the region ends where the longer one ends, Z / phiff / the shared region contiguous (ResLds: img_len is
//       their length), and `total` equal to what the structs gave before they moved here (the recorded file)
//   (b) every row of kResInst / kTileInst holds every N of its range within its max_lds_kb; the headline case is 81 488 bytes
//   (c) the word maps of the scratchpad, per set of roles that run together: words distinct, inside the scratchpad, every index
//       function inside the group of its name and type, mailboxes below the first named word, the staged constants at 64 and 70,
//       the derived zero list equal to the words marked zero (and to the list the prologue wrote out by hand)
//   (d) the launch word: unpack after pack returns the fields; the packed value equals the expression the launch sites wrote out
// The size of a region is what its kernel indexes.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../vi_ekf_amd/csrc/viekf_fused_lds.hpp"

namespace {

using namespace viekf;

enum Life { ALWAYS, PROP, UPD };
struct Region { const char* name; int at; std::size_t size; Life life; };   // doubles

long g_cases = 0, g_bad = 0;
std::map<std::tuple<std::string, int, int, std::size_t>, int> g_recorded;

void fail(const char* what, int N, std::size_t ctx, const char* msg, const char* r1 = "", const char* r2 = "") {
  if (g_bad++ < 16) std::printf("FAIL %s N=%d ctx_bytes=%zu: %s %s %s\n", what, N, ctx, msg, r1, r2);
}

int even(std::size_t c) { return (int)((c + 1) & ~(std::size_t)1); }

void check_regions(const char* what, int N, std::size_t ctx, const std::vector<Region>& rs, int total) {
  for (std::size_t i = 0; i < rs.size(); i++) {
    const Region& r = rs[i];
    if (r.at < 0 || r.at + r.size > (std::size_t)total) fail(what, N, ctx, "region outside total:", r.name);
    if (r.at % 2 != 0) fail(what, N, ctx, "region off a 16-byte boundary:", r.name);
    for (std::size_t j = i + 1; j < rs.size(); j++) {
      const Region& s = rs[j];
      const bool together = r.life == ALWAYS || s.life == ALWAYS || r.life == s.life;
      if (together && r.size && s.size && r.at < s.at + (int)s.size && s.at < r.at + (int)r.size) fail(what, N, ctx, "regions overlap:", r.name, s.name);
    }
  }
}

void check_recorded(const char* family, int N, int staged, std::size_t ctx, int total) {
  const auto it = g_recorded.find({family, N, staged, ctx});
  if (it == g_recorded.end()) fail(family, N, ctx, "no recorded total");
  else if (it->second != total) fail(family, N, ctx, "total differs from the recorded one");
}

void check_res(int N, bool staged, std::size_t cb) {
  g_cases++;
  const int nx = 17 + 5 * N, nxs = (nx + 1) & ~1, n = 16 + 3 * N, nf = 3 * N, mc = res_mcap(N);   // (as viekf_batch_create sets them)
  const std::size_t un = (std::size_t)n, uN = (std::size_t)N, zlen = (std::size_t)(nf * ZS > 4 * n ? nf * ZS : 4 * n);
  const ResLds L(N, n, nxs, staged, cb);
  const std::vector<Region> rs = {
      {"xs", L.xs, (std::size_t)nxs, ALWAYS}, {"lam", L.lam, un, ALWAYS}, {"sm", L.sm, (std::size_t)res_sm::len(staged), ALWAYS},
      {"fixadd", L.fixadd, 2 * uN, ALWAYS}, {"fixset", L.fixset, 2 * uN, ALWAYS}, {"Z", L.Z, zlen, ALWAYS}, {"phiff", L.phiff, 9 * uN, ALWAYS},
      {"Abb", L.Abb, 256, PROP}, {"Gb", L.Gb, 96, PROP}, {"Phibb", L.Phibb, 256, PROP}, {"PhibbT", L.PhibbT, 256, PROP}, {"Gdb", L.Gdb, 96, PROP},
      {"T16", L.T16, 256, PROP}, {"PsiP", L.PsiP, (std::size_t)ZK * 16, PROP}, {"Pi", L.Pi, (std::size_t)ZK * ZK, PROP}, {"Xi", L.Xi, (std::size_t)ZK * 16, PROP},
      {"AvG", L.AvG, 18, PROP},
      {"Kt", L.Kt, 2 * un, UPD}, {"Wt", L.Wt, 2 * un, UPD}, {"Praw", L.Praw, 4 * un > 256 ? 4 * un : 256, UPD}, {"Pd", L.Pd, 4 * uN, UPD},
      {"Mbb", L.Mbb, 256, ALWAYS}, {"Pbb", L.Pbb, 256, ALWAYS}, {"xdb", L.xdb, 16, ALWAYS}, {"ctx", L.ctx, (cb + 7) / 8, ALWAYS},
      {"Pbc", L.Pbc, (std::size_t)nf * 16, ALWAYS}, {"Lbc", L.Lbc, 48, ALWAYS},
      {"mslot", L.mslot, (std::size_t)mc / 2, ALWAYS}, {"mseq", L.mseq, (std::size_t)mc, ALWAYS}, {"mz", L.mz, 2 * (std::size_t)mc, ALWAYS}, {"mR", L.mR, 4 * (std::size_t)mc, ALWAYS}};
  const char* what = staged ? "ResLds(staged)" : "ResLds";
  check_regions(what, N, cb, rs, L.total);
  // one region, two lives
  if (L.Abb != L.Kt) fail(what, N, cb, "the two lives start apart");
  const int endp = L.AvG + even(18), endu = L.Pd + even(4 * uN), end = endp > endu ? endp : endu;
  if (L.Mbb != end) fail(what, N, cb, "the shared region does not end with its longer life");
  if (L.Z + even(zlen) != L.phiff || L.phiff + even(9 * uN) != L.Abb) fail(what, N, cb, "Z, phiff and the shared region are not contiguous");
  if (L.img_len != end - L.Z) fail(what, N, cb, "img_len is not the length of Z .. the shared region");
  check_recorded("res", N, staged ? 1 : 0, cb, L.total);
}

void check_tile(int N, std::size_t cb) {
  g_cases++;
  const int nx = 17 + 5 * N, nxs = (nx + 1) & ~1, n = 16 + 3 * N, nf = 3 * N, mc = res_mcap(N), NQ = 16 * tile_nt(N);
  const std::size_t un = (std::size_t)n, uN = (std::size_t)N;
  const TileLds L(N, n, nxs, cb);
  const std::vector<Region> rs = {
      {"xs", L.xs, (std::size_t)nxs, ALWAYS}, {"lam", L.lam, un, ALWAYS}, {"sm", L.sm, (std::size_t)tile_sm::len(), ALWAYS},
      {"fixadd", L.fixadd, 2 * uN, ALWAYS}, {"fixset", L.fixset, 2 * uN, ALWAYS}, {"Z", L.Z, (std::size_t)nf * ZS, ALWAYS}, {"phiff", L.phiff, 9 * uN, ALWAYS},
      {"Abb", L.Abb, 256, PROP}, {"Gb", L.Gb, 96, PROP}, {"Phibb", L.Phibb, 256, PROP}, {"PhibbT", L.PhibbT, 256, PROP}, {"Gdb", L.Gdb, 96, PROP},
      {"T16", L.T16, 256, PROP}, {"PsiP", L.PsiP, (std::size_t)ZK * 16, PROP}, {"Pi", L.Pi, (std::size_t)ZK * ZK, PROP}, {"Xi", L.Xi, (std::size_t)ZK * 16, PROP},
      {"AvG", L.AvG, 18, PROP},
      {"Cb", L.Cb, 4 * (std::size_t)NQ, UPD}, {"Eb", L.Eb, 4 * (std::size_t)NQ, UPD}, {"Pd", L.Pd, 4 * uN, UPD},
      {"Mbb", L.Mbb, 256, ALWAYS}, {"Pbb", L.Pbb, 256, ALWAYS}, {"xdb", L.xdb, 16, ALWAYS}, {"ctx", L.ctx, (cb + 7) / 8, ALWAYS},
      {"Pbc", L.Pbc, (std::size_t)nf * 16, ALWAYS},
      {"mslot", L.mslot, (std::size_t)mc / 2, ALWAYS}, {"mseq", L.mseq, (std::size_t)mc, ALWAYS}, {"mz", L.mz, 2 * (std::size_t)mc, ALWAYS}, {"mR", L.mR, 4 * (std::size_t)mc, ALWAYS}};
  check_regions("TileLds", N, cb, rs, L.total);
  if (L.Abb != L.Cb) fail("TileLds", N, cb, "the two lives start apart");
  const int endp = L.AvG + even(18), endu = L.Pd + even(4 * uN), end = endp > endu ? endp : endu;
  if (L.Mbb != end) fail("TileLds", N, cb, "the shared region does not end with its longer life");
  if (L.Z + even((std::size_t)nf * ZS) != L.phiff || L.phiff + even(9 * uN) != L.Abb) fail("TileLds", N, cb, "Z, phiff and the shared region are not contiguous");
  if (L.pair_word(1, tile_sm::TRIPS) != L.total + L.sm + 60 || L.pair_word(0, tile_sm::TRIPS) != L.sm + 60) fail("TileLds", N, cb, "the pair's trip counts moved");
  check_recorded("tile", N, 0, cb, L.total);
}

// ---- word maps ----
template <int NWD>
const SmWords* group_of(const SmWords (&words)[NWD], int w) {
  for (const SmWords& g : words)
    if (w >= g.at && w < g.at + g.count) return &g;
  return nullptr;
}
template <int NWD>
void expect_word(const char* what, const SmWords (&words)[NWD], int w, const char* name, bool is_int, unsigned cfg) {
  const SmWords* g = group_of(words, w);
  if (!g || std::strcmp(g->name, name) != 0) fail(what, w, 0, "index function outside its group:", name);
  else if (g->is_int != is_int) fail(what, w, 0, "type of the word differs:", name);
  else if (!(g->live & cfg)) fail(what, w, 0, "word used where the map says nobody reads it:", name);
}
template <int NWD>
void check_words(const char* what, const SmWords (&words)[NWD], unsigned cfg, int len, int first_mbox_end, int mbox_stride, int mbox_fields) {
  g_cases++;
  std::vector<int> owner(256, -1);
  int first_named = len;
  for (int i = 0; i < NWD; i++) {   // (every group, also those nobody reads in this configuration: their positions are taken)
    const SmWords& g = words[i];
    if (g.at < 0 || g.at + g.count > len) fail(what, g.at, 0, "words outside the scratchpad:", g.name);
    for (int w = g.at; w < g.at + g.count && w < 256; w++) {
      if (owner[w] >= 0) fail(what, w, 0, words[owner[w]].is_int != g.is_int ? "an int and a double share a word:" : "words overlap:", g.name, words[owner[w]].name);
      owner[w] = i;
    }
    if ((g.live & cfg) && std::strncmp(g.name, "mailbox ", 8) != 0 && g.at < first_named) first_named = g.at;   // (the sequence numbers count as named)
  }
  if (mbox_fields > mbox_stride) fail(what, 0, 0, "a mailbox reaches into the next one");
  if (first_mbox_end > first_named) fail(what, first_named, 0, "the mailboxes reach the first named word");
  // the derived zero list: exactly the words marked zero
  const unsigned long long mask = sm_zero_mask(words);
  for (int w = 0; w < 64; w++) {
    const bool marked = owner[w] >= 0 && words[owner[w]].zero;
    if (marked != (((mask >> w) & 1) != 0)) fail(what, w, 0, "the zero list and the words marked zero differ");
  }
}

void check_maps() {
  for (int two = 0; two < 2; two++) {
    const unsigned cfg = two ? SM_RES2 : SM_RES1;
    const char* what = two ? "res_sm (two service waves)" : "res_sm (one service wave)";
    check_words(what, res_sm::kWords, cfg, res_sm::len(true), res_sm::mbox(1) + res_sm::MB_FIELDS, res_sm::MB_STRIDE, res_sm::MB_FIELDS);
    for (const SmWords& g : res_sm::kWords)   // without the staged constants everything lies in the control block
      if ((g.live & cfg) && g.at < res_sm::CTRL_WORDS && g.at + g.count > res_sm::len(false)) fail(what, g.at, 0, "control word outside the unstaged scratchpad:", g.name);
    for (int phase = 0; phase < 12; phase++) {
      expect_word(what, res_sm::kWords, res_sm::gate_word(phase), "gate verdict", false, cfg);
      expect_word(what, res_sm::kWords, res_sm::nan_word(two ? 1 : 0, phase), "NaN guard", false, cfg);
      if (two) expect_word(what, res_sm::kWords, res_sm::nan_word(2, phase), "NaN guard, body wave", false, cfg);
      if (res_sm::nan_word(0, phase) != res_sm::nan_word(0, phase + 3) || res_sm::gate_word(phase) != res_sm::gate_word(phase + 2)) fail(what, phase, 0, "period of a phase word");
    }
    for (int par = 0; par < 2; par++) {
      expect_word(what, res_sm::kWords, res_sm::fix_word(two ? 1 : 0, par), "fix mailbox non-empty", false, cfg);
      if (two) expect_word(what, res_sm::kWords, res_sm::fix_word(2, par), "fix mailbox non-empty, body wave", false, cfg);
      if (two) expect_word(what, res_sm::kWords, res_sm::mbox_seq(par), "mailbox sequence numbers", true, cfg);
      if (two) expect_word(what, res_sm::kWords, res_sm::mbox(par) + res_sm::MB_GATE, par ? "mailbox 1" : "mailbox 0", false, cfg);
    }
    expect_word(what, res_sm::kWords, res_sm::DT, "dt", false, cfg);
  }
  {   // the list the prologue wrote out by hand before the map: the same stores, so the same kernels
    unsigned long long hand = 0;
    for (int w : {40, 41, 44, 45, 46, 49, 50, 51, 32, 33, 52, 53, 54, 36, 37}) hand |= 1ull << w;
    if (sm_zero_mask(res_sm::kWords) != hand) fail("res_sm", 0, 0, "the zero list differs from the hand-written one");
    for (const SmWords& g : res_sm::kWords)   // every word somebody reads before anybody writes it is on it; what is on it beyond those is dead
      if (!g.zero && g.live && std::strcmp(g.name, "dt") != 0 && g.at < res_sm::CTRL_WORDS && std::strncmp(g.name, "mailbox ", 8) != 0) fail("res_sm", g.at, 0, "a control word that is not cleared:", g.name);
  }
  if (res_sm::SQRTQU != 64 || res_sm::QXB != 70) fail("res_sm", 0, 0, "the staged constants moved");
  if (res_sm::len(false) != 64 || res_sm::len(true) != 86 || tile_sm::len() != 64) fail("sm", 0, 0, "length of a scratchpad");
  // positions as the kernels have had them
  if (res_sm::mbox(1) != 16 || res_sm::mbox_seq(1) != 33 || res_sm::fix_word(2, 1) != 37 || res_sm::fix_word(0, 1) != 41 || res_sm::fix_word(1, 0) != 40 ||
      res_sm::DT != 42 || res_sm::nan_word(0, 2) != 46 || res_sm::nan_word(1, 4) != 45 || res_sm::nan_word(2, 5) != 54 || res_sm::gate_word(3) != 51)
    fail("res_sm", 0, 0, "a word moved");
  if (tile_sm::mbox(1) != 8 || tile_sm::MB_SKIP != 3 || tile_sm::fix_word(1) != 41 || tile_sm::DT != 42 || tile_sm::nan_word(5) != 46 || tile_sm::TRIPS != 60)
    fail("tile_sm", 0, 0, "a word moved");
  for (int pair = 0; pair < 2; pair++) {
    const unsigned cfg = pair ? SM_TILE_PAIR : SM_TILE;
    const char* what = pair ? "tile_sm (pair)" : "tile_sm (single)";
    check_words(what, tile_sm::kWords, cfg, tile_sm::len(), tile_sm::mbox(1) + tile_sm::MB_FIELDS, tile_sm::MB_STRIDE, tile_sm::MB_FIELDS);
    for (int phase = 0; phase < 12; phase++) expect_word(what, tile_sm::kWords, tile_sm::nan_word(phase), "NaN in the column pair", false, cfg);
    for (int par = 0; par < 2; par++) {
      expect_word(what, tile_sm::kWords, tile_sm::fix_word(par), "fix mailbox non-empty", false, cfg);
      expect_word(what, tile_sm::kWords, tile_sm::mbox(par) + tile_sm::MB_SKIP, par ? "mailbox 1" : "mailbox 0", false, cfg);
    }
    expect_word(what, tile_sm::kWords, tile_sm::DT, "dt", false, cfg);
    if (pair) expect_word(what, tile_sm::kWords, tile_sm::TRIPS, "updates that will run", false, cfg);
  }
}

void check_launch_word() {
  g_cases++;
  for (int prop = 0; prop < 2; prop++)
    for (int fmt = 0; fmt < 8; fmt++)
      for (int KP = 1; KP <= 64; KP++)
        for (int dbg = 0; dbg < 256; dbg++) {
          const int w = launch_pack(prop != 0, KP, fmt, dbg);
          const int recorded = (prop ? (1 | (KP << 16)) : 0) | (fmt << 1) | ((dbg & 0xff) << 8);   // launch_resident, before
          if (w != recorded) fail("launch word", KP, 0, "packed value differs from the recorded expression");
          // (KP travels with the propagate bit: a launch without a propagate reads 1)
          if (launch_prop(w) != prop || launch_fmt(w) != fmt || launch_dbg(w) != dbg || launch_kp(w) != (prop ? KP : 1)) fail("launch word", KP, 0, "unpack after pack");
        }
  if (launch_pack(false, 1, RES_FMT_LOAD_PACKED | RES_FMT_P_ONLY, 0) != ((RES_FMT_LOAD_PACKED | RES_FMT_P_ONLY) << 1)) fail("launch word", 0, 0, "unpack_buffer's word");   // before
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: fused_lds_model RECORDED_TOTALS\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  char line[256];
  while (std::fgets(line, sizeof line, f)) {
    char fam[16];
    int N, staged, total;
    std::size_t cb;
    if (line[0] != '#' && std::sscanf(line, "%15s %d %d %zu %d", fam, &N, &staged, &cb, &total) == 5) g_recorded[{fam, N, staged, cb}] = total;
  }
  std::fclose(f);

  const std::size_t ctx_sizes[] = {kBodyCtxBytes, 436, 444, 4, 8, 12, 1028};   // (the sizes tests/cpp/stream_lds_model.cpp uses)
  for (std::size_t cb : ctx_sizes) {
    for (int N = 1; N <= 77; N++)
      for (int staged = 0; staged < 2; staged++) check_res(N, staged != 0, cb);
    for (int N = 1; N + 14 <= 64; N++) check_tile(N, cb);
  }
  if (g_recorded.size() != 7 * (77 * 2 + 50)) fail("recorded totals", 0, 0, "number of recorded lines");

  // every dispatch row holds its whole range (setup_resident / setup_tiles decide by this), with the real BodyCtx
  for (const ResInst& r : kResInst) {
    g_cases++;
    for (int N = r.nmin; N <= r.nmax; N++) {
      const ResLds L(N, 16 + 3 * N, (17 + 5 * N + 1) & ~1, res_batched_loads(r.RB, r.NW), kBodyCtxBytes);
      if (sizeof(double) * (std::size_t)L.total > (std::size_t)r.max_lds_kb * 1024) fail("kResInst row", N, kBodyCtxBytes, "past max_lds_kb");
    }
  }
  for (const TileInst& r : kTileInst) {
    g_cases++;
    for (int N = 1; N + 14 <= 64; N++) {
      if (tile_nt(N) != r.NT) continue;
      const TileLds L(N, 16 + 3 * N, (17 + 5 * N + 1) & ~1, kBodyCtxBytes);
      if (sizeof(double) * (std::size_t)L.total * (r.pair ? 2 : 1) > (std::size_t)r.max_lds_kb * 1024) fail("kTileInst row", N, kBodyCtxBytes, "past max_lds_kb");
    }
  }
  {   // the headline: <7, 3> at N = 50 (the comment above res_mcap)
    const ResLds L(50, 166, 268, res_batched_loads(7, 3), kBodyCtxBytes);
    if (sizeof(double) * (std::size_t)L.total != 81488) fail("headline", 50, kBodyCtxBytes, "not 81 488 bytes");
  }
  check_maps();
  check_launch_word();

  std::printf("cases %ld failures %ld\n", g_cases, g_bad);
  if (g_bad) { std::printf("fused lds model: FAILED\n"); return 1; }
  std::printf("fused lds model: ok\n");
  return 0;
}
