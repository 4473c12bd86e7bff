// Model check of the dynamic-LDS layouts of the streaming-side kernels (vi_ekf_amd/csrc/viekf_stream_lds.hpp), stand-alone on a
// CPU: the header is plain C++17, this program includes nothing else of the library.  For every feature count N = 0 .. 512, with
// nx / nxs / n as viekf_batch_create sets them, and for several sizes of BodyCtx (odd multiples of 4 bytes among them), every
// struct is checked for three things:
//   (a) its regions are pairwise disjoint and lie inside bytes()
//   (b) every region of doubles starts on an 8-byte boundary
//   (c) bytes() equals the RECORDED FORMULA: the expression the launch site of the kernel used before the layouts were stated
//       once, written out literally below -- a launch must ask for exactly the bytes it always asked for.
// The size of a region is what its kernel indexes (the comments of the header's fields).
// The layouts of the wide-P path (WideLds, BlkLds at groups of 16 / 24 / 32, PsvLds at 16) are checked the same way, their named
// int sub-regions included (4-byte boundaries), and the regions a kernel reads as double2 (the panel's rows, the S^-1 columns, pzz,
// ctab) for 16-byte boundaries; their recorded formula is the sum of `take`s of the constructor each struct had in its kernel's
// header.  grouped_choice -- which grouped update a batch gets -- is held, for every N and every tuning combination, to the
// dispatch logic it replaced (written out literally below) and to what the kernels take for granted of a choice; a few choices are
// pinned by value.
#include <cstddef>
#include <cstdio>
#include <vector>

#include "../../vi_ekf_amd/csrc/viekf_stream_lds.hpp"

namespace {

struct Region { const char* name; std::size_t at, size; bool doubles; bool pairs = false; };   // bytes; pairs: read as double2

long g_cases = 0, g_bad = 0;

void fail(const char* layout, int N, std::size_t ctx, const char* what, const char* r1, const char* r2 = "") {
  if (g_bad++ < 12) std::printf("FAIL %s N=%d ctx_bytes=%zu: %s %s %s\n", layout, N, ctx, what, r1, r2);
}

void check(const char* layout, int N, std::size_t ctx, const std::vector<Region>& regions, std::size_t bytes, std::size_t recorded) {
  g_cases++;
  for (std::size_t i = 0; i < regions.size(); i++) {
    const Region& r = regions[i];
    if (r.at + r.size > bytes) fail(layout, N, ctx, "region past bytes():", r.name);
    if (r.doubles && r.at % 8 != 0) fail(layout, N, ctx, "doubles off an 8-byte boundary:", r.name);
    if (!r.doubles && r.at % 4 != 0) fail(layout, N, ctx, "words off a 4-byte boundary:", r.name);
    if (r.pairs && r.at % 16 != 0) fail(layout, N, ctx, "double2 reads off a 16-byte boundary:", r.name);
    for (std::size_t j = i + 1; j < regions.size(); j++) {
      const Region& s = regions[j];
      if (r.size && s.size && r.at < s.at + s.size && s.at < r.at + r.size) fail(layout, N, ctx, "regions overlap:", r.name, s.name);
    }
  }
  if (bytes != recorded) fail(layout, N, ctx, "bytes() differs from the recorded formula", "");
}

Region dbl(const char* name, int at, std::size_t count) { return {name, sizeof(double) * (std::size_t)at, sizeof(double) * count, true}; }
Region dbl2(const char* name, int at, std::size_t count) { return {name, sizeof(double) * (std::size_t)at, sizeof(double) * count, true, true}; }
Region ints(const char* name, int at, std::size_t count) { return {name, sizeof(double) * (std::size_t)at, sizeof(int) * count, false}; }

// ---- the constructors the three wide-P structs had in their kernels' headers, as sums of their `take`s (doubles)
std::size_t ev(std::size_t c) { return (c + 1) & ~(std::size_t)1; }
std::size_t recorded_wide(std::size_t N, std::size_t nxs, std::size_t cb) {
  return ev(nxs) + ev(256) + ev(96) + ev(256) + ev(256) + ev(256) + ev(96) + ev(256) + ev(256) + ev(16) + ev((cb + 7) / 8) + ev(18) +
         ev(9 * 16) + ev(9 * 9) + ev(9 * 16) + ev(9 * N) + ev(3 * N * 26) + ev(8);
}
std::size_t recorded_blk(std::size_t N, std::size_t n, std::size_t nxs, std::size_t BG) {
  const std::size_t nr = (n + 15) & ~(std::size_t)15, BLD = 2 * BG + 2, BWIN = 2 * BG;
  return ev(nxs) + ev(n) + ev(nr * BLD) + ev(4 * BG) + ev(32) + ev(N > 0 ? N : 1) + ev(2 * BG) + ev(7 * BWIN);
}
std::size_t recorded_psv(std::size_t N, std::size_t n, std::size_t nxs, std::size_t BG) {
  const std::size_t nr = (n + 15) & ~(std::size_t)15, BLD = 2 * BG + 2, BWIN = 2 * BG;
  return ev(nxs) + ev(n) + ev(nr * BLD) + ev(4 * BG) + ev(2 * 12 * BG) + ev(2 * (4 * BG * (BG - 1) / 2)) + ev(2 * 6 * BG) + ev(6 * BG) + ev(2) +
         ev(N > 0 ? N : 1) + ev(2 * BG) + ev(2 * 7 * BWIN);
}

// ---- panel_svc / blocked_group of viekf_dispatch.hpp as they stood before grouped_choice: kind 0 none, 1 blocked, 2 panelsvc
struct OldChoice { int kind, BG; std::size_t bytes; };
OldChoice old_choice(int N, int n, int nxs, int tune_block_group, int tune_panel_svc, int tune_stream_mfma) {
  const std::size_t psv_bytes = sizeof(double) * recorded_psv(N, n, nxs, 16);
  const bool panel_svc = !(tune_panel_svc == 0 || !(tune_block_group == 0 || tune_block_group == 16) || n > 512) &&
                         psv_bytes + 1024 <= 160 * 1024;
  if (tune_stream_mfma == 0 || n > 512) return {0, 0, 0};
  if (panel_svc) return {2, 16, psv_bytes};
  auto fits = [&](int cand, std::size_t* bytes) {
    *bytes = sizeof(double) * recorded_blk(N, n, nxs, cand);
    return *bytes + 1024 <= 160 * 1024;
  };
  std::size_t bytes = 0;
  if (tune_block_group && fits(tune_block_group, &bytes)) return {1, tune_block_group, bytes};
  for (int cand : {32, 24, 16}) {
    if (cand > 16 && n <= 256) continue;
    if (fits(cand, &bytes)) return {1, cand, bytes};
  }
  return {0, 0, 0};
}

void expect(bool ok, const char* what, int N, int a = 0, int b = 0, int c = 0) {
  g_cases++;
  if (!ok && g_bad++ < 12) std::printf("FAIL choice N=%d tuning (%d, %d, %d): %s\n", N, a, b, c, what);
}

}  // namespace

int main() {
  using namespace viekf;
  const std::size_t ctx_sizes[] = {440, 436, 444, 4, 8, 12, 1028};   // 440 = today's BodyCtx (55 doubles)
  for (int N = 0; N <= 512; N++) {
    const int nx = 17 + 5 * N, nxs = (nx + 1) & ~1, n = 16 + 3 * N;
    const std::size_t un = (std::size_t)n, unxs = (std::size_t)nxs;
    for (std::size_t cb : ctx_sizes) {
      for (int mf = 0; mf < 2; mf++) {
        const PropLds L(nxs, cb, N, mf != 0);
        // the launch sites of k_propagate_stream: lds_propagate(b), and "+ 9 N + 2 doubles" for the matrix-core instance
        std::size_t recorded = sizeof(double) * (std::size_t)(nxs + 256 + 96 + 256 + 256 + 96 + 256 + 256 + 16) + cb + 16;
        if (mf) recorded += sizeof(double) * (9 * (std::size_t)N + 2);
        check(mf ? "PropLds(mf)" : "PropLds", N, cb,
              {dbl("xs", L.xs, unxs), dbl("Abb", L.Abb, 256), dbl("Gb", L.Gb, 96), dbl("Phibb", L.Phibb, 256), dbl("Mbb", L.Mbb, 256),
               dbl("Gdb", L.Gdb, 96), dbl("Pbb", L.Pbb, 256), dbl("T16", L.T16, 256), dbl("xdb", L.xdb, 16),
               {"ctx", sizeof(double) * (std::size_t)L.ctx, cb, true}, dbl("Dl", L.Dl, mf ? 9 * (std::size_t)N : 0)},
              L.bytes(), recorded);
      }
      const XdotLds X(nxs, cb);
      check("XdotLds", N, cb,
            {dbl("xs", X.xs, unxs), dbl("Abb", X.Abb, 256), dbl("Gb", X.Gb, 96), dbl("xdb", X.xdb, 16),
             {"ctx", sizeof(double) * (std::size_t)X.ctx, cb, true}},
            X.bytes(), sizeof(double) * (std::size_t)(nxs + 256 + 96 + 16) + cb + 16);   // viekf_batch_eval_xdot
    }
    const UpdLds U(nxs, n);
    check("UpdLds", N, 0, {dbl("xs", U.xs, unxs), dbl("W", U.W, 2 * un), dbl("K", U.K, 2 * un), dbl("lam", U.lam, un), dbl("sm", U.sm, 32)},
          U.bytes(), sizeof(double) * (std::size_t)(nxs + 5 * n + 32));                   // lds_update(b)
    const GenLds G(nxs, n);
    check("GenLds", N, 0, {dbl("xs", G.xs, unxs), dbl("W", G.W, 3 * un), dbl("K", G.K, 3 * un), dbl("lam", G.lam, un), dbl("sm", G.sm, 64)},
          G.bytes(), sizeof(double) * (std::size_t)(nxs + 7 * n + 64));                   // viekf_batch_update
    for (std::size_t cb : ctx_sizes) {
      const WideLds W(N, nxs, cb);
      check("WideLds", N, cb,
            {dbl("xs", W.xs, unxs), dbl("Abb", W.Abb, 256), dbl("Gb", W.Gb, 96), dbl("Phibb", W.Phibb, 256), dbl("PhibbT", W.PhibbT, 256),
             dbl("Mbb", W.Mbb, 256), dbl("Gdb", W.Gdb, 96), dbl("Pbb", W.Pbb, 256), dbl("T16", W.T16, 256), dbl("xdb", W.xdb, 16),
             {"ctx", sizeof(double) * (std::size_t)W.ctx, cb, true}, dbl("AvG", W.AvG, 18), dbl("PsiP", W.PsiP, ZK * 16), dbl("Pi", W.Pi, ZK * ZK),
             dbl("Xi", W.Xi, ZK * 16), dbl("phiff", W.phiff, 9 * (std::size_t)N), dbl("Z", W.Z, 3 * (std::size_t)N * ZS), dbl("sm", W.sm, 8)},
            W.bytes(), sizeof(double) * recorded_wide(N, nxs, cb));
    }
    const std::size_t nr = (un + 15) & ~(std::size_t)15, nd = N > 0 ? N : 1;
    for (int BG : {16, 24, 32}) {
      const BlkLds L(N, n, nxs, BG);
      const std::size_t g = BG, bw = 2 * g;
      if (L.BLD != 2 * BG + 2 || L.BWIN != 2 * BG || L.BLD % 2) fail("BlkLds", N, 0, "BLD / BWIN", "");
      check(BG == 16 ? "BlkLds<16>" : (BG == 24 ? "BlkLds<24>" : "BlkLds<32>"), N, 0,
            {dbl("xs", L.xs, unxs), dbl("lam", L.lam, un), dbl2("Wp", L.Wp, nr * L.BLD), dbl2("Si", L.Si, 4 * g), dbl2("pzz", L.pzz, 8),
             ints("badf", L.badf, g), dbl("diag", L.diag, nd), ints("gsl", L.gsl, g), ints("gml", L.gml, g), dbl("wz", L.wz, 2 * bw),
             dbl("wR", L.wR, 4 * bw), ints("wsl", L.wsl, bw)},
            L.bytes(), sizeof(double) * recorded_blk(N, n, nxs, BG));
    }
    {
      const int BG = 16;
      const PsvLds L(N, n, nxs, BG);
      const std::size_t g = BG, bw = 2 * g;
      if (L.mail_sz != 12 * BG || L.ctab_sz != 4 * BG * (BG - 1) / 2 || L.cbuf_sz != 6 * BG || L.mail_sz % 2 || L.ctab_sz % 2)
        fail("PsvLds", N, 0, "sizes per parity", "");
      check("PsvLds<16>", N, 0,
            {dbl("xs", L.xs, unxs), dbl("lam", L.lam, un), dbl2("Wp", L.Wp, nr * L.BLD), dbl2("Si", L.Si, 4 * g),
             dbl("mail[0]", L.mail, L.mail_sz), dbl("mail[1]", L.mail + L.mail_sz, L.mail_sz), dbl2("ctab[0]", L.ctab, L.ctab_sz),
             dbl2("ctab[1]", L.ctab + L.ctab_sz, L.ctab_sz), dbl("cbuf[0]", L.cbuf, L.cbuf_sz), dbl("cbuf[1]", L.cbuf + L.cbuf_sz, L.cbuf_sz),
             dbl("cpre", L.cpre, L.cbuf_sz), ints("spec", L.spec, 2), ints("ticket", L.ticket, 1), dbl("diag", L.diag, nd),
             ints("gsl[0]", L.gsl, g), ints("gml[0]", L.gml, g), ints("gsl[1]", L.gsl + L.slot_stride, g), ints("gml[1]", L.gml + L.slot_stride, g),
             dbl("wz[0]", L.wz, 2 * bw), dbl("wR[0]", L.wR, 4 * bw), ints("wsl[0]", L.wsl, bw), dbl("wz[1]", L.wz + L.win_stride, 2 * bw),
             dbl("wR[1]", L.wR + L.win_stride, 4 * bw), ints("wsl[1]", L.wsl + L.win_stride, bw)},
            L.bytes(), sizeof(double) * recorded_psv(N, n, nxs, BG));
    }
    // ---- the choice, for every tuning combination
    for (int tbg : {0, 16, 24, 32})
      for (int tps : {0, 1})
        for (int tmf : {0, 1, 2}) {
          const GroupedChoice c = grouped_choice(N, n, nxs, tbg, tps, tmf);
          const OldChoice o = old_choice(N, n, nxs, tbg, tps, tmf);
          const int kind = c.kernel == GroupedKernel::none ? 0 : (c.kernel == GroupedKernel::blocked ? 1 : 2);
          bool ok = kind == o.kind && c.BG == o.BG && c.bytes == o.bytes;
          if (kind != 0) {   // what the kernels take for granted: a row per thread, the three slot masks, the LDS budget
            ok = ok && n <= 512 && N <= 192 && c.bytes + 1024 <= 160 * 1024 && (c.BG == 16 || c.BG == 24 || c.BG == 32);
            ok = ok && c.bytes == (kind == 2 ? PsvLds(N, n, nxs, c.BG).bytes() : BlkLds(N, n, nxs, c.BG).bytes());
            if (kind == 2) ok = ok && 3 * c.BG <= 64 && N <= 512 - 65;   // a group's rows on one wave; thread T - 65 past every feature
          } else
            ok = ok && c.BG == 0 && c.bytes == 0;
          expect(ok, "differs from the dispatch logic it replaced, or breaks what a kernel assumes", N, tbg, tps, tmf);
        }
    // ---- pinned: the default takes the look-ahead kernel up to N = 154 and the blocked one from 155 (while a panel fits at all)
    {
      const GroupedChoice c = grouped_choice(N, n, nxs, 0, 1, 1);
      if (N <= 154) expect(c.kernel == GroupedKernel::panelsvc && c.BG == 16, "default: panelsvc up to N = 154", N, 0, 1, 1);
      else if (N <= 160) expect(c.kernel == GroupedKernel::blocked && c.BG == 16, "default: blocked<16> from N = 155", N, 0, 1, 1);
      else expect(c.kernel != GroupedKernel::panelsvc, "default: no panelsvc past N = 154", N, 0, 1, 1);
    }
    if (N == 17 || N == 85 || N == 100) {   // the blocked rows of tests/hetero_cases.py (panel service 0)
      const GroupedChoice c = grouped_choice(N, n, nxs, 0, 0, 1);
      expect(c.kernel == GroupedKernel::blocked && c.BG == (N == 17 ? 16 : (N == 85 ? 32 : 24)), "pinned blocked group size", N, 0, 0, 1);
    }
    const KeepLds Kp(n);
    check("KeepLds", N, 0,
          {{"colbuf", Kp.colbuf, sizeof(double) * un, true}, {"srcrow", Kp.srcrow, sizeof(int) * un, false}, {"cnt", Kp.cnt, sizeof(int), false}},
          Kp.bytes(), sizeof(double) * (std::size_t)n + sizeof(int) * (std::size_t)(n + 4));   // viekf_batch_keep_features, viekf_frame_update
  }
  std::printf("cases %ld failures %ld\n", g_cases, g_bad);
  if (g_bad) { std::printf("stream lds model: FAILED\n"); return 1; }
  std::printf("stream lds model: ok\n");
  return 0;
}
