// viekf_kernels_grouped.hpp -- the GROUPED feature updates of the wide-P path (P in HBM, 77 < N <= 160; forced at any N by the
// streaming family): P crosses HBM once per group of up to BG measurements instead of once per measurement.
//   k_update_feat_blocked<512, 16 | 24 | 32>   r03: a group walked measurement by measurement by the whole workgroup, then one
//                                              pass over P (blk_pass).  Runs forced group sizes, N > 154 and A/B comparisons.
//   k_update_feat_panelsvc<512, 16>            r04, the default: the sequential part of a group on ONE service wave, a group
//                                              ahead, under the previous group's pass (psv_pass).
// The two passes are different algorithms on purpose and so are the corrections from stored W rows (the
// look-ahead kernel writes its multiply-adds out so that the service wave and the row owners round alike).
//
// Defines kernels: included from viekf_dispatch.hpp only.  The dynamic-LDS carve-ups (BlkLds, PsvLds) and the choice between the
// two kernels (grouped_choice) are in viekf_stream_lds.hpp, plain C++ that tests/cpp/stream_lds_model.cpp checks on a CPU.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_onepass.hpp"
#include "viekf_resident_prop.hpp"
#include "viekf_stream_lds.hpp"

namespace viekf {

// ------------------------------------------------------------------------------------------------
// M sequential active FEAT updates, BLOCKED for a covariance that does not fit on chip (wide P): the same arithmetic
// as k_update_feat_stream, but P crosses HBM once per GROUP of up to BG measurements instead of once per measurement.
//   1. panel:  the 2 zeta columns of every feature measured in the group, all rows, -> LDS  (n x 2 BG)
//   2. for each measurement of the group, in order: innovation, gate, W = panel_g Hb^T (in place), K = W S^-1 (in
//      registers; only S^-1 is kept), state correction, fix_depth; the rank-2 update is applied to the LATER panel columns
//      only (they are all that the following gains need) and to an exact running copy of the rho-rho diagonal (fix_depth
//      edits it, vi_ekf_helper.cpp:128-156, and a "set" does not commute with later updates).
//   3. one pass over P:  P -= Lambda o (K W^T)  with W = n x 2 BG from LDS and K = W S^-1 re-formed on the fly -- a dense
//      contraction, done per 16x16 tile by v_mfma_f64_16x16x4_f64 (BG/2 k-steps), Lambda applied to the accumulator; the
//      rho-rho diagonal takes the running copy.
// A slot that repeats inside a group starts a new group.  HBM traffic per step drops from (M+1) to (M/BG+1) passes over P;
// keeping W alone (K costs two multiply-adds per operand instead of 127 KB of LDS) is what lets BG = 16 fit at N = 160.
// LDS rows of W are 34 doubles apart: the MFMA operand reads (16 consecutive rows per k) then spread over the banks.
// ------------------------------------------------------------------------------------------------
// One pass over P:  P -= Lambda o (K W^T), 16 x 16 tiles on the fp64 matrix cores.
//      D[r][c] = sum_k W[j0+r][k] K[i0+c][k]:  D's column index (lane & 15) runs along the ROWS of P (contiguous in memory).
// (the pass of k_update_feat_blocked alone: the look-ahead kernel has its own, psv_pass below)
template <int T, int BLD>
__device__ __forceinline__ void blk_pass(double* __restrict__ P, int ld, int nact, int Gn, const double* Wp, const double* SiL,
                                         const double* lam, const double* diag, bool partial, int lane, int wave) {
  constexpr int NWV = T / 64;
    const int nt = (nact + 15) >> 4;
    const int lr = lane & 15, lk = lane >> 4;
    const int ksteps = (2 * Gn + 3) >> 2;               // (columns past 2 Gn are zero)
    constexpr int TPI = 8;   // tiles per wave and unit: their 32 loads of P are in flight together (one tile at a time
                             // leaves 2 KB per wave on the wire and the pass latency-bound at a fraction of the HBM rate)
    // P stays EXACTLY symmetric and is read only once per pair: the tiles on and below the diagonal are processed; a diagonal
    // tile forms K_i . W_j for i >= j and the mirror expression K_j . W_i (same products, same order) for i < j.
    // Work unit of a wave: TPI vertically adjacent tiles of one column block (rows 16 ti0 .. +127): its loads cover 1024
    // contiguous bytes per column (HBM likes long runs: 128-byte runs scattered over the matrix reached 2.8 TB/s).  Units
    // are numbered column block by column block over the lower triangle and dealt to the waves round-robin.
    struct Unit { int tj, ti0; };
    auto next_unit = [&](Unit u, int steps) {            // advance `steps` units (past the end: tj == nt)
      for (int s2 = 0; s2 < steps && u.tj < nt; s2++) {
        u.ti0 += TPI;
        if (u.ti0 >= nt) { u.tj++; u.ti0 = u.tj; }
      }
      return u;
    };
    auto load_tiles = [&](Unit u, double (&pq)[TPI][4]) {
      const int tj = min(u.tj, nt - 1);                  // (clamped, unconditional loads: branch-free, so the compiler can
#pragma unroll                                             //  count them exactly instead of draining the queue at every use)
      for (int q = 0; q < TPI; q++) {
        const int i = min(16 * (u.ti0 + q) + lr, nact - 1);
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int j = min(16 * tj + lk + 4 * rg, nact - 1);
          pq[q][rg] = P[i + (long)j * ld];
        }
      }
    };
    double pv[TPI][4];
    Unit u = next_unit(Unit{0, 0}, wave);
    while (u.tj < nt) {
      load_tiles(u, pv);                // (the SIMD's other wave computes meanwhile; an explicit prefetch of the next unit
      const Unit un = next_unit(u, NWV);   //  did not pay for its registers)
      const int tj = u.tj, j0t = 16 * tj;
#pragma unroll
      for (int q = 0; q < TPI; q++) {
        const int ti = u.ti0 + q;
        if (ti >= nt) break;
        const int i0 = 16 * ti;
        const bool diag_t = ti == tj;
        v4f64 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
        for (int sk = 0; sk < ksteps; sk++) {
          const int c = 4 * sk + lk;                       // this lane's contraction index: column c of pair c >> 1
          const double wjc = Wp[(j0t + lr) * BLD + c];
          const double2 wi = *reinterpret_cast<const double2*>(Wp + (i0 + lr) * BLD + (c & ~1));
          const double2 sv = *reinterpret_cast<const double2*>(SiL + 4 * (c >> 1) + 2 * (c & 1));
          const double kic = wi.x * sv.x + wi.y * sv.y;    // K[i][c], the same expression as in the panel phase
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wjc, kic, acc, 0, 0, 0);                          // K_i . W_j
          if (diag_t) {                                    // (wave-uniform)
            const double2 wj = *reinterpret_cast<const double2*>(Wp + (j0t + lr) * BLD + (c & ~1));
            const double wic = (c & 1) ? wi.y : wi.x;
            const double kjc = wj.x * sv.x + wj.y * sv.y;
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(kjc, wic, acc2, 0, 0, 0);                      // K_j . W_i
          }
        }
        if (diag_t) {
#pragma unroll
          for (int rg = 0; rg < 4; rg++)
            if (i0 + lr < j0t + lk + 4 * rg) acc[rg] = acc2[rg];   // upper triangle of the diagonal tile
        }
        const int i = i0 + lr;
        const double li = lam[min(i, nact - 1)];
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {                   // (results stay in pv: every store is issued after the last
          const int j = j0t + lk + 4 * rg;                 //  wait on a load -- a store ahead of a load wait would be waited for too)
          const double lj = lam[min(j, nact - 1)];
          const double Lij = partial ? (lj + li - li * lj) : 1.0;
          double v = pv[q][rg] - Lij * acc[rg];
          if (i == j && i >= 16 && i < nact && (i - 16) % 3 == 2) v = diag[(i - 16) / 3];
          pv[q][rg] = v;
        }
      }
#pragma unroll
      for (int q = 0; q < TPI; q++) {
        const int ti = u.ti0 + q;
        const int i = 16 * ti + lr;
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int j = 16 * tj + lk + 4 * rg;
          if (ti < nt && i < nact && j < nact) {
            P[i + (long)j * ld] = pv[q][rg];   // (no mirror store: nothing reads above the diagonal, see the panel load)
          }
        }
      }
      u = un;
    }
}

// ------------------------------------------------------------------------------------------------
// What the two kernels do alike, stated once (each adopted where the kernel's listing keeps its registers and its floating-point,
// matrix-core, LDS and global-memory instruction counts: profiles/grouped/README.md).
// ------------------------------------------------------------------------------------------------
// Stages the window [m, m + BWIN) of filter b's measurement list in LDS (one parallel fetch instead of a chain of dependent global
// loads) and decides each entry's admission: wsl = its slot, or -1 with the code written to the results -- -1 for a slot < 0, 3
// (MEAS_INVALID) for a slot the filter does not track, 2 (MEAS_NAN, vi_ekf_meas.cpp:136-137) for a NaN pixel.  Threads 0 .. BWIN - 1.
template <int BWIN>
__device__ __forceinline__ void group_stage_window(int tid, int b, int m, int M, int len, const double* __restrict__ z_all,
                                                   const int* __restrict__ slot_all, const double* __restrict__ R_all, long r_stride_b,
                                                   long r_stride_m, int* __restrict__ result_all, double* wz, double* wR, int* wsl) {
  if (tid < BWIN && m + tid < M) {
    const long mi = (long)b * M + m + tid;
    const int slot = slot_all[mi];
    const double z0 = z_all[2 * mi], z1 = z_all[2 * mi + 1];
    int code = 0;
    if (slot < 0) code = -1;
    else if (slot >= len) code = 3;                   // MEAS_INVALID
    else if (z0 != z0 || z1 != z1) code = 2;          // MEAS_NAN (vi_ekf_meas.cpp:136-137)
    wsl[tid] = code == 0 ? slot : -1;
    wz[2 * tid] = z0; wz[2 * tid + 1] = z1;
    const double* R = R_all + (long)b * r_stride_b + (long)(m + tid) * r_stride_m;   // column-major 2x2
    wR[4 * tid] = R[0]; wR[4 * tid + 1] = R[1]; wR[4 * tid + 2] = R[2]; wR[4 * tid + 3] = R[3];
    if (code != 0 && result_all) result_all[mi] = code;
  }
}

// Scans the staged window from entry m for the next group: up to `cap` admitted entries with distinct slots; a repeated slot ends
// the group (it opens the next), so does the window's end `mend`.  Every thread scans the same words (uniform control flow); tid 0
// records slot and window index of each member.  -> the group's size; mm: the entry the scan stopped at; s0..s2: the group's slots
// as a set (3 x 64 >= the 160-feature limit: grouped_choice holds N <= 192)
__device__ __forceinline__ int group_scan(int tid, const int* wsl, int m, int mend, int cap, int* gsl, int* gml, int& mm,
                                          unsigned long long& s0, unsigned long long& s1, unsigned long long& s2) {
  int Gn = 0;
  mm = m;
  while (mm < mend && Gn < cap) {
    const int slot = wsl[mm - m];
    if (slot >= 0) {
      unsigned long long& w = slot < 64 ? s0 : (slot < 128 ? s1 : s2);
      const unsigned long long bit = 1ull << (slot & 63);
      if (w & bit) break;                             // repeated slot: it opens the next group
      w |= bit;
      if (tid == 0) { gsl[Gn] = slot; gml[Gn] = mm - m; }   // (index into the window)
      Gn++;
    }
    mm++;
  }
  return Gn;
}

// panel <- the zeta columns of the group's features, one row per thread trip; unused columns <- 0.  Only the LOWER triangle of P is
// valid: element (i, c) of a column comes from the column where i >= c (coalesced along the rows) and from ROW c where i < c (one
// 8-byte read per thread, a column apart; the rows of a group's features are mostly neighbours -- measurements arrive in slot order
// -- so a thread's reads share 128-byte lines).  That costs about a quarter of a pass in fetched lines per group and saves the
// mirrored stores of every pass (r02: up to the whole upper triangle per pass, the kernel's largest single write stream) and the
// propagate's transpose pass.  CH: the independent column loads in flight per thread and trip over the row's NC = 2 BG columns.
template <int T, int BLD, int NC, int CH>
__device__ __forceinline__ void group_load_panel(const double* __restrict__ P, int ld, int nact, int Gn, const int* gsl, double* Wp, int tid) {
  for (int i = tid; i < nact; i += T) {
#pragma unroll 1
    for (int c0 = 0; c0 < NC; c0 += CH) {
      double v[CH];
#pragma unroll
      for (int k = 0; k < CH; k++) {
        const int c = c0 + k;
        const int col = 16 + 3 * gsl[(c < 2 * Gn) ? (c >> 1) : 0] + (c & 1);
        v[k] = (c < 2 * Gn) ? P[max(i, col) + (long)min(i, col) * ld] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < CH; k += 2) *reinterpret_cast<double2*>(Wp + i * BLD + c0 + k) = make_double2(v[k], v[k + 1]);
    }
  }
}

// The pass's S^-1 operand of one measurement: the two COLUMNS of S^-1 = {Si[0], Si[2] | Si[1], Si[3]} (row-major Si in)
__device__ __forceinline__ void group_pack_si(double* SiL4, const double* Si) {
  SiL4[0] = Si[0]; SiL4[1] = Si[2]; SiL4[2] = Si[1]; SiL4[3] = Si[3];
}

// The launch's last words: the state back to memory, scanned for NaN / blow-up; the filter's flags
template <int T>
__device__ __forceinline__ void group_store_state(const double* xs, double* __restrict__ xg, int len, int tid, unsigned flag, unsigned* flags_b) {
  for (int i = tid; i < xZ + 5 * len; i += T) {
    const double v = xs[i];
    if (v != v) flag |= FLAG_NAN;
    if (v > 1e6) flag |= FLAG_BLOWUP;
    xg[i] = v;
  }
  if (flag) atomicOr(flags_b, flag);
}

// ------------------------------------------------------------------------------------------------
// BG = measurements per group (template parameter: 16, 24 or 32 -- the largest whose panel fits the LDS, so that the narrower
// filters of this family cross HBM fewer times); BLD = 2 BG + 2 = LDS row stride (doubles) of the n x 2 BG panel; BWIN = 2 BG
// measurement-list entries staged per group.  The LDS carve-up: BlkLds (viekf_stream_lds.hpp).
// Where a kernel below needs several regions of one set -- the slots of a group (gsl, gml), a staged window (wz, wR, wsl) -- it
// forms ONE pointer from the set's first field and reaches the others by the DIFFERENCE of two layout fields (in doubles; x 2 for
// an int pointer): a compile-time constant once BG is one, so the set is addressed off one register.  Formed each from its own
// field the look-ahead kernel came out two VGPRs larger (profiles/grouped/README.md).
template <int T, int BG>
__global__ __launch_bounds__(T) void k_update_feat_blocked(StreamArgs a, const double* __restrict__ z_all,
                                                           const int* __restrict__ slot_all, int M,
                                                           const double* __restrict__ R_all, long r_stride_b,
                                                           long r_stride_m, int* __restrict__ result_all) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  if (a.active && !a.active[b]) return;
  const int n = a.n, ld = a.ld;
  constexpr int BLD = 2 * BG + 2, BWIN = 2 * BG;
  const BlkLds L(a.N, n, a.nxs, BG);
  double* xs = smem + L.xs;
  double* lam = smem + L.lam;
  double* Wp = smem + L.Wp;     // panel of raw columns, turned into W pair by pair
  double* SiL = smem + L.Si;    // per pair g: {Si00, Si10, Si01, Si11} = the two COLUMNS of S^-1 (zero if the update was skipped)
  double* pzz = smem + L.pzz;   // [2][4] zeta-zeta block of the current / next measurement
  int* badf = reinterpret_cast<int*>(smem + L.badf);   // [BG] NaN-guard verdict of each measurement of the group (set by any thread)
  double* diag = smem + L.diag; // running P(rho_f, rho_f)
  int* gsl = reinterpret_cast<int*>(smem + L.gsl);
  int* gml = gsl + 2 * (L.gml - L.gsl);
  double* wz = smem + L.wz;
  double* wR = wz + (L.wR - L.wz);
  int* wsl = reinterpret_cast<int*>(wz + (L.wsl - L.wz));
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const DevParams& prm = a.prm(b);
  const bool partial = prm.use_partial_update != 0;
  unsigned flag = 0;
  constexpr int NWV = T / 64;
  const int lane = tid & 63, wave = tid >> 6;

  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lam(b)[i];
  __syncthreads();

  int m = 0, mbase = 0;
  while (m < M) {
    // ---- stage a window of the measurement list, then form the next group from it
    __syncthreads();   // (the previous group is done with the window)
    group_stage_window<BWIN>(tid, b, m, M, len, z_all, slot_all, R_all, r_stride_b, r_stride_m, result_all, wz, wR, wsl);
    __syncthreads();
    int mm;
    unsigned long long seen0 = 0, seen1 = 0, seen2 = 0;   // (the group's slots as a set: not needed past the scan here)
    const int Gn = group_scan(tid, wsl, m, min(M, m + BWIN), BG, gsl, gml, mm, seen0, seen1, seen2);
    mbase = m;
    m = mm;
    if (Gn == 0) continue;
    // ---- 1. panel <- the zeta columns of the group's features, eight independent column loads in flight per thread
    group_load_panel<T, BLD, 2 * BG, 8>(P, ld, nact, Gn, gsl, Wp, tid);
    if (tid < 4 * BG) SiL[tid] = 0.0;
    if (tid < BG) badf[tid] = 0;
    for (int f = tid; f < len; f += T) diag[f] = P[(16 + 3 * f + 2) + (long)(16 + 3 * f + 2) * ld];
    // The zeta-zeta 2x2 of the measurement about to be processed is handed over in pzz[parity][4] by the two threads that own
    // its rows (they are the ones that keep those panel entries current), so nobody reads panel rows that are being rewritten.
    const int i = tid;                                      // this thread's row of the panel (T >= n: grouped_choice)
    // Lambda of (this row, a bearing column):  lambda_i + lambda_c - lambda_i lambda_c  with the bearing components' lambda_c
    double Lza = 1.0, Lzb = 1.0;
    if (partial) { const double li = lam[min(i, n - 1)], la = lam[16], lb = lam[17]; Lza = la + li - li * la; Lzb = lb + li - li * lb; }
    auto publish_pzz = [&](int gn) {                        // for measurement gn of the group, from the thread's own row
      if (gn < Gn) {
        const int jn = 16 + 3 * gsl[gn];
        if (i == jn || i == jn + 1)
          *reinterpret_cast<double2*>(pzz + 4 * (gn & 1) + 2 * (i - jn)) = *reinterpret_cast<const double2*>(Wp + i * BLD + 2 * gn);
      }
    };
    auto fix_depth_own = [&]() {                            // fix_depth (:271) on the state and the running diagonal
      for (int f = tid; f < len; f += T) fix_depth_diag(xs, diag, f, prm, flag);
    };
    publish_pzz(0);   // (own row: written by this thread in the load above)
    __syncthreads();
    // ---- 2. the measurements of the group, in order; two barriers each
    for (int g = 0; g < Gn; g++) {
      const int slot = gsl[g], wi = gml[g];
      int* res = result_all ? &result_all[(long)b * M + mbase + wi] : nullptr;
      const double* R = wR + 4 * wi;                                // column-major 2x2
      // prediction, innovation, S^-1 and the gate: every thread for itself (uniform data; cheaper than a broadcast + barrier)
      double zhat[2], Hb[4];
      {
        double t1[3], t2[3], zt[3];
        bearing_frame_fast(xs + xZ + 5 * slot, t1, t2, zt);
        h_feat_frame(t1, t2, zt, prm, zhat, Hb);
      }
      const double h00 = Hb[0], h01 = Hb[1], h10 = Hb[2], h11 = Hb[3];
      const double r0 = wz[2 * wi] - zhat[0], r1 = wz[2 * wi + 1] - zhat[1];   // residual (vi_ekf_meas.cpp:220)
      double Si[4];
      const double* pz = pzz + 4 * (g & 1);
      const double mahal = feat_innovation(Hb, pz[0], pz[1], pz[2], pz[3], R, r0, r1, Si);   // vi_ekf_meas.cpp:230-234
      if (mahal > kGateMahal) {                                   // gate (:235-239): returns before fix_depth
        if (res && tid == 0) *res = 1;
        if (i < nact) *reinterpret_cast<double2*>(Wp + i * BLD + 2 * g) = make_double2(0.0, 0.0);
        publish_pzz(g + 1);
        __syncthreads();
        continue;
      }
      int bad = 0;
      double k0 = 0.0, k1 = 0.0;                           // this thread's row of K
      if (i < nact) {                                      // W = P H^T, K = W S^-1 (:241), NaN guard (:247)
        const double2 pr = *reinterpret_cast<const double2*>(Wp + i * BLD + 2 * g);
        const double w0 = pr.x * h00 + pr.y * h01, w1 = pr.x * h10 + pr.y * h11;
        k0 = w0 * Si[0] + w1 * Si[2]; k1 = w0 * Si[1] + w1 * Si[3];
        *reinterpret_cast<double2*>(Wp + i * BLD + 2 * g) = make_double2(w0, w1);
        if (k0 != k0 || k1 != k1) bad = 1;
      }
      if (h00 != h00 || h01 != h01 || h10 != h10 || h11 != h11) bad = 1;
      if (bad) badf[g] = 1;                                // (a flag word and ONE barrier: __syncthreads_or is a workgroup reduction,
      __syncthreads();                                     //  two barriers and an LDS round trip per measurement)
      bad = badf[g];                                       // barrier 1: the W pair is complete
      if (bad) {
        if (i < nact) *reinterpret_cast<double2*>(Wp + i * BLD + 2 * g) = make_double2(0.0, 0.0);
      } else {
        if (tid == 0) group_pack_si(SiL + 4 * g, Si);
        // state correction  x <- x [+] (lambda o K r)   (:254-255 / :262-263);  K rows re-formed from W where needed
        auto krow = [&](int row, double& q0, double& q1) {
          const double2 w = *reinterpret_cast<const double2*>(Wp + row * BLD + 2 * g);
          q0 = w.x * Si[0] + w.y * Si[2]; q1 = w.x * Si[1] + w.y * Si[3];
        };
        if (tid == T - 1) {                                // (a thread without a feature of its own: T >= n > len, grouped_choice)
          double dxb[16], xo[17];
#pragma unroll
          for (int q = 0; q < 16; q++) {
            const double l = partial ? lam[q] : 1.0;
            double q0, q1;
            krow(q, q0, q1);
            dxb[q] = (l * q0) * r0 + (l * q1) * r1;
          }
          body_boxplus_fast(xs, dxb, xo);
#pragma unroll
          for (int q = 0; q < 17; q++) xs[q] = xo[q];
        }
        for (int f = tid; f < len; f += T) {
          const int d = 16 + 3 * f;
          double dv[3], k2[2] = {0.0, 0.0};
#pragma unroll
          for (int q = 0; q < 3; q++) {
            const double l = partial ? lam[d + q] : 1.0;
            double q0, q1;
            krow(d + q, q0, q1);
            dv[q] = (l * q0) * r0 + (l * q1) * r1;
            k2[0] = q0; k2[1] = q1;
          }
          double qn[4];
          q_feat_boxplus_fast(xs + xZ + 5 * f, dv[0], dv[1], qn);
          double* xf = xs + xZ + 5 * f;
          xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
          xf[4] += dv[2];
          // running rho-rho diagonal:  P_ii -= Lambda_ii (K_i . W_i)
          const int ir = d + 2;
          const double li = lam[ir];
          const double Lii = partial ? (li + li - li * li) : 1.0;
          const double2 wr = *reinterpret_cast<const double2*>(Wp + ir * BLD + 2 * g);
          diag[f] -= Lii * (k2[0] * wr.x + k2[1] * wr.y);
        }
        // the later panel columns follow the update:  P_ic -= Lambda_ic (K_i . W_c), this thread's row
        // Four column pairs per trip, their operands loaded together: one pair at a time is a chain of LDS round trips (the
        // compiler keeps every load behind the previous pair's store), about a quarter of the measurement's latency at 16 per group.
        // (The mask of a (row, bearing column) pair is the same for every feature: lambda_feat is one triple for all slots.)
        if (i < nact) {
#pragma unroll 1
          for (int gc0 = g + 1; gc0 < Gn; gc0 += 4) {
            double2 wa[4], wb[4], pc[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
              const int gc = min(gc0 + q, Gn - 1);
              const int cr = 16 + 3 * gsl[gc];
              wa[q] = *reinterpret_cast<const double2*>(Wp + cr * BLD + 2 * g);
              wb[q] = *reinterpret_cast<const double2*>(Wp + (cr + 1) * BLD + 2 * g);
              pc[q] = *reinterpret_cast<const double2*>(Wp + i * BLD + 2 * gc);
            }
#pragma unroll
            for (int q = 0; q < 4; q++) {
              if (gc0 + q < Gn) {
                pc[q].x -= Lza * (k0 * wa[q].x + k1 * wa[q].y);
                pc[q].y -= Lzb * (k0 * wb[q].x + k1 * wb[q].y);
                *reinterpret_cast<double2*>(Wp + i * BLD + 2 * (gc0 + q)) = pc[q];
              }
            }
          }
        }
      }
      fix_depth_own();                                     // (not gated: runs after a NaN-guarded update too, :271)
      publish_pzz(g + 1);
      if (res && tid == 0) *res = 0;
      __syncthreads();                                     // barrier 2: state, panel and pzz are ready for the next measurement
    }
    // ---- 3. one pass over P:  P -= Lambda o (K W^T), 16 x 16 tiles on the fp64 matrix cores (blk_pass above)
    blk_pass<T, BLD>(P, ld, nact, Gn, Wp, SiL, lam, diag, partial, lane, wave);
    __syncthreads();
  }
  group_store_state<T>(xs, xg, len, tid, flag, &a.flags[b]);
}


// ------------------------------------------------------------------------------------------------
// k_update_feat_panelsvc (r04): the grouped feature update of the wide-P path (k_update_feat_blocked above:
// the same panel of zeta columns in LDS, the same one pass over P per group of 16 measurements) with the SEQUENTIAL part of a group
// reduced to what is sequential -- the way a blocked factorisation treats its diagonal block -- and run one group AHEAD, under the
// previous group's pass over P.
// VIEKF::update for active FEAT measurements, src/vi_ekf/vi_ekf_meas.cpp:196-278 (h_feat :354-367, gate :230-239, K :241, NaN
// guard :247, partial update :249-258, fix_depth :271), applied in the caller's order.
//
// k_update_feat_blocked walks a group measurement by measurement with the whole workgroup: every thread runs the prediction /
// S^-1 / gate chain, forms its W row, (barrier) applies the update to the later panel columns of its row, (barrier): 7,400 clk
// = 3.1 us per measurement at N = 150 (tools/stamps_wide.py), during which the CU moves no byte of P -- 150 x 3.1 us x 4 dispatch
// rounds = 1.9 of the 7.3 ms of a step.  But measurement g + 1 needs from update g only (i) the state of ITS feature and (ii) the
// 2 x 2 zeta-zeta block of ITS feature: the rows of the group's own features.  So, per group G:
//   S. ONE wave (the last) runs the chain of the whole group alone, without a barrier: lane l holds panel row 16 + 3 f_q + c of group
//      feature q = l / 3, component c = l % 3 -- all 32 columns of it, in registers -- and the state of feature q; per measurement:
//      prediction / S^-1 / gate from lane values (v_readlane), W and K of the 48 rows, the later columns of those rows, the state
//      correction and fix_depth of the 16 group features (one instruction stream for all of them).  It leaves {Hb, S^-1, r, gate}
//      per measurement and the W values of the later features' zeta rows (the coupling every other row needs) in LDS.
//      It does so WHILE THE OTHER SEVEN WAVES RUN THE PASS OF GROUP G - 1: its 48 x 32 entries of P are read before that pass starts
//      and brought up to date by the wave itself from the W rows of group G - 1 (the same rank-32 correction the pass applies), as
//      are the states of its 16 features.
//   A. (after the pass) the panel of group G is loaded;  C. every thread brings ITS panel row up to date on its own: the same
//      recurrence over g with the row in registers, the couplings read from LDS -- no barrier, no panel traffic -- and stores its W
//      row; the NaN guard (:247) is checked on every row's K here.
//   D. The state of the features outside groups G and G + 1 and of the body follows from the stored W rows, measurement by measurement,
//      on the lanes that own them (no barrier either), then the pass of group G (under which S of group G + 1 runs).
// S speculates that no update of the group is NaN-guarded (it cannot know: the verdict needs every row).  Nothing is committed before
// C has checked: if a K turned out NaN the group is run again as groups of ONE measurement, where the verdict is exact before anything
// is applied (the update is then skipped, fix_depth runs, :247,271).  Rows: one per thread (T >= n).  BG = 16: 48 rows fit the wave.
// The service wave's copy of its 48 x 32 entries equals what the pass writes up to rounding (it sums the same products in another
// order): the chain's S^-1 and couplings carry that rounding, nothing else does -- P itself is only ever written by the pass.
// ------------------------------------------------------------------------------------------------
// W row = panel row x Hb^T and K row = W row x S^-1 with the multiply-adds written out: the service wave and the row owners
// round the same way
__device__ __forceinline__ void psv_wk(double px, double py, const double* hb, const double* si, double& w0, double& w1, double& k0, double& k1) {
  w0 = fma(px, hb[0], py * hb[1]);
  w1 = fma(px, hb[2], py * hb[3]);
  k0 = fma(w0, si[0], w1 * si[2]);
  k1 = fma(w0, si[1], w1 * si[3]);
}
__device__ __forceinline__ double psv_sub(double p, double nk0, double nk1, double wx, double wy) {   // p - L (K_i . W_c), nk = -L K_i
  return fma(nk0, wx, fma(nk1, wy, p));
}
__device__ __forceinline__ double psv_rl(double v, int src) {   // lane src's value for the whole wave (v_readlane, lands in SGPRs)
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int psv_tri(int g, int gp, int BG) { return g * BG - g * (g + 1) / 2 + (gp - g - 1); }   // g < gp

// The pass of the look-ahead kernel:  P -= Lambda o (K W^T)  on the lower triangle, 16 x 16 tiles on the fp64 matrix cores, like
// blk_pass above -- but r04 measured that pass to be LATENCY-bound, not HBM-bound (B = 64 filters, a quarter of the
// traffic and all of it cache-resident, take 1.66 ms per step against 1.76 ms at B = 256): a wave walks its tiles one by one, every
// k-step a chain of three LDS reads -> K -> one MFMA into the same accumulator.  Here a wave works on FOUR tiles of a unit at a time: the
// four accumulator chains are independent, and the W rows of the unit's column block and the S^-1 columns -- the same for every tile of
// the unit -- are read once per k-step instead of once per tile and k-step (6 LDS reads per 4 MFMAs instead of 12).  The diagonal tiles
// (both orientations, second accumulator) are units of their own and keep the one-tile form.  Units are drawn from an LDS counter.
template <int T, int BLD>
__device__ __forceinline__ void psv_pass(double* __restrict__ P, int ld, int nact, int Gn, const double* Wp, const double* SiL,
                                         const double* lam, bool partial, int lane, int* ticket,
                                         unsigned long long* st = nullptr) {
  const int nt = (nact + 15) >> 4;
  const int lr = lane & 15, lk = lane >> 4;
  const int ksteps = (2 * Gn + 3) >> 2;                   // (columns past 2 Gn are zero)
#ifdef VIEKF_STAMPS
  int sn = 0;                                             // diagnostic build: the first sixteen marks of this wave's pass
#define PASS_STAMP()                                                                      \
  do {                                                                                    \
    if (st && sn < 16) {                                                                   \
      __builtin_amdgcn_sched_barrier(0);                                                  \
      if (lane == 0) st[sn] = __builtin_amdgcn_s_memtime();                               \
      __builtin_amdgcn_sched_barrier(0);                                                  \
      sn++;                                                                               \
    }                                                                                     \
  } while (0)
#else
#define PASS_STAMP() do {} while (0)
#endif
  constexpr int TPI = 4;                                  // tiles per unit: 4 vertically adjacent ones (512 B contiguous per column)
  int NU = 0;                                             // units strictly below the diagonal: tickets 0 .. NU - 1, then the nt diagonal tiles
  for (int tj = 0; tj < nt; tj++) NU += (nt - 1 - tj + TPI - 1) / TPI;
  auto draw = [&]() {
    int t = 0;
    if (lane == 0) t = atomicAdd(ticket, 1);
    return __builtin_amdgcn_readfirstlane(t);
  };
  // ---- a unit strictly below the diagonal: column block tj, tiles ti0 .. ti0 + 3
  auto decode = [&](int t, int& tj, int& ti0) {
    int rest = t;
    for (tj = 0; tj < nt; tj++) {
      const int nu = (nt - 1 - tj + TPI - 1) / TPI;       // units of this column block (rows tj + 1 .. nt - 1)
      if (rest < nu) break;
      rest -= nu;
    }
    ti0 = tj + 1 + TPI * rest;
  };
  // the matrix-core work of a unit and the Lambda scaling: pv -= Lambda o (K_I . W_J^T)
  auto compute = [&](double (&pv)[TPI][4], int tj, int ti0) {
    const int j0t = 16 * tj;
    v4f64 acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = v4f64{0.0, 0.0, 0.0, 0.0};
    int ib[4];
#pragma unroll
    for (int q = 0; q < 4; q++) ib[q] = min(16 * (ti0 + q), 16 * (nt - 1)) + lr;   // (a tile past the end redoes the last one)
    for (int sk = 0; sk < ksteps; sk++) {                  // (two waves of a SIMD in this loop at once are bound by the matrix core:
      const int c = 4 * sk + lk;                           //  reading the next k-step's operands ahead gained nothing, r04)
      const double wjc = Wp[(j0t + lr) * BLD + c];         // this lane's contraction index: column c of pair c >> 1
      const double2 sv = *reinterpret_cast<const double2*>(SiL + 4 * (c >> 1) + 2 * (c & 1));
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const double2 wi = *reinterpret_cast<const double2*>(Wp + ib[q] * BLD + (c & ~1));
        const double kic = wi.x * sv.x + wi.y * sv.y;      // K[i][c]
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(wjc, kic, acc[q], 0, 0, 0);   // K_i . W_j
      }
    }
    PASS_STAMP();
    double lj[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) lj[rg] = lam[min(j0t + lk + 4 * rg, nact - 1)];
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const double li = lam[min(ib[q], nact - 1)];
#pragma unroll
      for (int rg = 0; rg < 4; rg++) {
        const double Lij = partial ? (lj[rg] + li - li * lj[rg]) : 1.0;
        pv[q][rg] -= Lij * acc[q][rg];
      }
    }
    PASS_STAMP();
  };
  PASS_STAMP();
  int t = draw();
  if (ld >= 16 * nt) {
    // Padded columns (the streaming family's layout, viekf_capi.hip: ld a multiple of 16): every row 16 ti + lr < 16 nt of a column
    // below n exists in memory, and the panel rows nact .. 16 nt - 1 are ZERO (written once per launch), so the ragged last tile row
    // needs neither clamps nor predicates -- the update of its rows past nact is  P -= Lambda o (0 . W^T): the value read is written
    // back.  A unit is then 16 loads and 16 stores at 32-bit offsets from the workgroup's base (the address arithmetic and the
    // predicates were a quarter of a unit's time), and the loop is software-pipelined over two register sets: the loads of the NEXT
    // unit are issued before the matrix-core work of the current one.  (A unit of fewer than four tiles redoes its last tile in the
    // spare slots: the same values stored twice.)  Nothing branches between a load and its use: a join makes the compiler's
    // wait-count bookkeeping wait for BOTH sets.
    auto offs = [&](int tj, int ti0, int q, int rg) {
      return (unsigned)(min(16 * (ti0 + q), 16 * (nt - 1)) + lr) + (unsigned)(16 * tj + lk + 4 * rg) * (unsigned)ld;
    };
    auto issue = [&](int tt, double (&pv)[TPI][4], int& tj, int& ti0) {
      decode(tt, tj, ti0);
#pragma unroll
      for (int q = 0; q < TPI; q++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) pv[q][rg] = P[offs(tj, ti0, q, rg)];
    };
    auto store = [&](const double (&pv)[TPI][4], int tj, int ti0) {
#pragma unroll
      for (int q = 0; q < TPI; q++)
#pragma unroll
        for (int rg = 0; rg < 4; rg++) P[offs(tj, ti0, q, rg)] = pv[q][rg];
      PASS_STAMP();
    };
    if (t < NU) {
      double pvA[TPI][4], pvB[TPI][4];
      int tjA, tiA, tjB, tiB;
      issue(t, pvA, tjA, tiA);
      PASS_STAMP();
      for (;;) {                                          // (the issue is unconditional -- past the last unit it reloads that one and
        t = draw();                                       //  drops it)
        PASS_STAMP();
        issue(min(t, NU - 1), pvB, tjB, tiB);
        PASS_STAMP();
        compute(pvA, tjA, tiA);
        store(pvA, tjA, tiA);
        if (t >= NU) break;
        t = draw();
        PASS_STAMP();
        issue(min(t, NU - 1), pvA, tjA, tiA);
        PASS_STAMP();
        compute(pvB, tjB, tiB);
        store(pvB, tjB, tiB);
        if (t >= NU) break;
      }
    }
  } else {
    // dense columns (the on-chip family's layout, when this kernel is forced at a small N): clamped loads, predicated stores
    for (; t < NU; t = draw()) {
      int tj, ti0;
      decode(t, tj, ti0);
      const int j0t = 16 * tj;
      double pv[TPI][4];
#pragma unroll
      for (int q = 0; q < TPI; q++) {
        const int i = min(16 * (ti0 + q) + lr, nact - 1);
#pragma unroll
        for (int rg = 0; rg < 4; rg++) pv[q][rg] = P[i + (long)min(j0t + lk + 4 * rg, nact - 1) * ld];
      }
      compute(pv, tj, ti0);
#pragma unroll
      for (int q = 0; q < TPI; q++) {
        const int i = 16 * (ti0 + q) + lr;
#pragma unroll
        for (int rg = 0; rg < 4; rg++) {
          const int j = j0t + lk + 4 * rg;
          if (ti0 + q < nt && i < nact && j < nact) P[i + (long)j * ld] = pv[q][rg];
        }
      }
    }
  }
  // ---- the diagonal tiles: K_i . W_j for i >= j and the mirror expression K_j . W_i (same products, same order) for i < j
  for (; t < NU + nt; t = draw()) {
    const int j0t = 16 * (t - NU), i = j0t + lr;
    double pv[4];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) pv[rg] = P[min(i, nact - 1) + (long)min(j0t + lk + 4 * rg, nact - 1) * ld];
    v4f64 acc = {0.0, 0.0, 0.0, 0.0}, acc2 = {0.0, 0.0, 0.0, 0.0};
    for (int sk = 0; sk < ksteps; sk++) {
      const int c = 4 * sk + lk;
      const double2 wi = *reinterpret_cast<const double2*>(Wp + i * BLD + (c & ~1));
      const double2 sv = *reinterpret_cast<const double2*>(SiL + 4 * (c >> 1) + 2 * (c & 1));
      const double wic = (c & 1) ? wi.y : wi.x;
      const double kic = wi.x * sv.x + wi.y * sv.y;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wic, kic, acc, 0, 0, 0);
      acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(kic, wic, acc2, 0, 0, 0);
    }
    const double li = lam[min(i, nact - 1)];
#pragma unroll
    for (int rg = 0; rg < 4; rg++) {
      const int j = j0t + lk + 4 * rg;
      const double lj = lam[min(j, nact - 1)];
      const double Lij = partial ? (lj + li - li * lj) : 1.0;
      const double av = (i < j) ? acc2[rg] : acc[rg];
      if (i < nact && j < nact) P[i + (long)j * ld] = pv[rg] - Lij * av;
    }
  }
}

// Diagnostic build only (-DVIEKF_STAMPS, tools/stamps_wide.py): s_memtime stamps of filter 0, lane 0 of every wave, into the
// workspace: [16 wave + idx], in the SECOND trip of the group loop (the first overlapped one)
#ifdef VIEKF_STAMPS
#define PSV_STAMP(idx)                                                                                          \
  do {                                                                                                          \
    if (b == 0 && lane == 0 && stamp_iter == 1) {                                                               \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
      reinterpret_cast<unsigned long long*>(a.ws)[16 * wave + (idx)] = __builtin_amdgcn_s_memtime();            \
      __builtin_amdgcn_sched_barrier(0);                                                                        \
    }                                                                                                           \
  } while (0)
#else
#define PSV_STAMP(idx) do {} while (0)
#endif

template <int T, int BG>
__global__ __launch_bounds__(T) void k_update_feat_panelsvc(StreamArgs a, const double* __restrict__ z_all,
                                                            const int* __restrict__ slot_all, int M,
                                                            const double* __restrict__ R_all, long r_stride_b,
                                                            long r_stride_m, int* __restrict__ result_all) {
  static_assert(3 * BG <= 64, "the rows of a group's features have to fit one wave");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  if (a.active && !a.active[b]) return;
  const int n = a.n, ld = a.ld;
  constexpr int BLD = 2 * BG + 2, BWIN = 2 * BG, NC = 2 * BG;
  constexpr int NWV = T / 64;
  const PsvLds L(a.N, n, a.nxs, BG);
  double* xs = smem + L.xs;
  double* lam = smem + L.lam;
  double* Wp = smem + L.Wp;     // panel of raw columns; after phase C: the W rows
  double* SiL = smem + L.Si;    // per pair g: the two COLUMNS of S^-1 (zero if the update was skipped): operand of the pass
  int* spec = reinterpret_cast<int*>(smem + L.spec);      // [parity] a K of the group came out NaN: the speculation failed
  int* ticket = reinterpret_cast<int*>(smem + L.ticket);  // the pass's unit counter
  double* diag = smem + L.diag; // running P(rho_f, rho_f), kept for the whole launch
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const DevParams& prm = a.prm(b);
  const bool partial = prm.use_partial_update != 0;
  unsigned flag = 0;
  const int lane = tid & 63, wave = tid >> 6;
  const bool svc = wave == NWV - 1;
  const double rho_reset = 1.0 / (2.0 * prm.min_depth), p0rr = prm.P0_feat[2];
#ifdef VIEKF_STAMPS
  int stamp_iter = -1;
#endif

  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lam(b)[i];
  for (int f = tid; f < len; f += T) diag[f] = P[(16 + 3 * f + 2) + (long)(16 + 3 * f + 2) * ld];
  for (int i = nact * BLD + tid; i < ((n + 15) & ~15) * BLD; i += T) Wp[i] = 0.0;   // the panel rows past the active ones stay zero (psv_pass)
  __syncthreads();

  // fix_depth (vi_ekf_helper.cpp:128-156) of one feature: rho and its P(rho, rho), both in the caller's registers
  auto fix_depth_v = [&](double& rho, double& prr) {
    fix_depth_rule(rho, rho_reset, flag, [&](double e2) { prr += e2; }, [&] { prr = p0rr; });
  };
  auto in_set = [](int f, unsigned long long s0, unsigned long long s1, unsigned long long s2) {
    return ((f < 64 ? s0 : (f < 128 ? s1 : s2)) >> (f & 63)) & 1ull;
  };
  auto krow = [&](int row, int g, const double* Si, double& q0, double& q1) {   // K row re-formed from the stored W row
    const double2 w = *reinterpret_cast<const double2*>(Wp + row * BLD + 2 * g);
    q0 = fma(w.x, Si[0], w.y * Si[2]); q1 = fma(w.x, Si[1], w.y * Si[3]);
  };

  // ---- group state: `cur` is the group being formed / processed, `prev` the one whose pass is pending
  int m = 0;                         // next entry of the measurement list
  int single_until = -1;             // below this index of the list the groups hold ONE measurement (a failed speculation is redone so)
  int pb = 0;                        // parity of cur's LDS buffers
  int Gn = 0, mbase = 0;             // cur: measurements, where its window starts in the list
  unsigned long long c0 = 0, c1 = 0, c2 = 0;        // cur's feature slots
  int Gp = 0;                        // prev: measurements (0: no pass pending)
  unsigned long long p0 = 0, p1 = 0, p2 = 0;        // prev's feature slots

  // forms the next group from a staged window of the list (group_stage_window, group_scan); all threads; two barriers inside
  auto form_group = [&]() {
    double* wz = smem + L.wz + pb * L.win_stride;
    double* wR = wz + (L.wR - L.wz);
    int* wsl = reinterpret_cast<int*>(wz + (L.wsl - L.wz));
    int* gsl = reinterpret_cast<int*>(smem + L.gsl + pb * L.slot_stride);
    int* gml = gsl + 2 * (L.gml - L.gsl);
    Gn = 0; c0 = 0; c1 = 0; c2 = 0;
    if (tid == 0) *ticket = 0;                             // (the unit counter of the coming pass)
    while (Gn == 0 && m < M) {
      __syncthreads();
      group_stage_window<BWIN>(tid, b, m, M, len, z_all, slot_all, R_all, r_stride_b, r_stride_m, result_all, wz, wR, wsl);
      if (tid == 0) spec[pb] = 0;
      __syncthreads();
      int mm;
      Gn = group_scan(tid, wsl, m, min(M, m + BWIN), (m < single_until) ? 1 : BG, gsl, gml, mm, c0, c1, c2);
      mbase = m;
      m = mm;
    }
    __syncthreads();                                      // gsl / gml visible
    // (every thread scanned the same LDS words: the results are wave-uniform, but the compiler cannot know -- say so, or every
    //  `g < Gn` below becomes an exec-mask branch and the unrolled rows go to scratch)
    Gn = __builtin_amdgcn_readfirstlane(Gn); m = __builtin_amdgcn_readfirstlane(m); mbase = __builtin_amdgcn_readfirstlane(mbase);
    auto uni64 = [](unsigned long long v) {
      const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
      return ((unsigned long long)hi << 32) | lo;
    };
    c0 = uni64(c0); c1 = uni64(c1); c2 = uni64(c2);
  };

  form_group();

  for (;;) {
#ifdef VIEKF_STAMPS
    stamp_iter++;
#endif
    PSV_STAMP(0);
    // the service wave's row of cur's 48 x 32 entries of P as they stand in memory NOW: read before the pending pass starts to
    // rewrite them.  (Assigned on every thread -- zeros on the other waves -- so that the registers are free again behind the barrier.)
    double sp[NC];
    {
      const int* gsl = reinterpret_cast<const int*>(smem + L.gsl + pb * L.slot_stride);
      const bool mine = svc && lane < 3 * Gn;
      const int fq = gsl[min(lane / 3, max(Gn, 1) - 1)];
      const int row = 16 + 3 * fq + (lane - 3 * (lane / 3));
#pragma unroll
      for (int c = 0; c < NC; c++) {
        const int col = 16 + 3 * gsl[(c < 2 * Gn) ? (c >> 1) : 0] + (c & 1);
        sp[c] = (mine && c < 2 * Gn) ? P[max(row, col) + (long)min(row, col) * ld] : 0.0;
      }
    }
    __syncthreads();
    // ================= S: the service wave runs cur's chain  ||  the others: prev's state corrections (D) and pass
    if (svc) {
      if (Gn > 0) {
        // (the chain is ONE wave's serial work next to seven waves of pass: it gets the issue slots it asks for)
        __builtin_amdgcn_s_setprio(3);
        double* mail = smem + L.mail + pb * L.mail_sz;
        double* ctab = smem + L.ctab + pb * L.ctab_sz;
        double* cbuf = smem + L.cbuf + pb * L.cbuf_sz;
        const double* wz = smem + L.wz + pb * L.win_stride;
        const double* wR = wz + (L.wR - L.wz);
        const int* gsl = reinterpret_cast<const int*>(smem + L.gsl + pb * L.slot_stride);
        const int* gml = gsl + 2 * (L.gml - L.gsl);
        const double* pmail = smem + L.mail + (pb ^ 1) * L.mail_sz;   // prev's
        const int sq_l = lane / 3, sc_l = lane - 3 * sq_l;
        const bool svalid = lane < 3 * Gn;
        const int fq = gsl[min(sq_l, Gn - 1)];
        const int row = 16 + 3 * fq + sc_l;
        const double li = lam[row];
        double La = 1.0, Lb = 1.0, l = 1.0, Lii = 1.0;
        if (partial) { const double la = lam[16], lb = lam[17]; La = la + li - li * la; Lb = lb + li - li * lb; l = li; Lii = li + li - li * li; }
        double sq[4], srho, sprr;                          // state and P(rho, rho) of this lane's feature (used on the lanes with c = 0)
        {
          const double* xf = xs + xZ + 5 * fq;
          sq[0] = xf[0]; sq[1] = xf[1]; sq[2] = xf[2]; sq[3] = xf[3]; srho = xf[4];
          sprr = diag[fq];
        }
        if (Gp > 0) {
          // prev's pass is pending: this lane's entries and its feature's state take prev's updates here (the same rank-2 terms the
          // pass applies / the corrections of D; a feature that was IN prev already has its state through prev)
          // (two loops -- the 48 x 32 entries, then the states -- so that the row, the operands in flight and the manifold step's
          //  temporaries are not all live at once)
#pragma unroll 1
          for (int g = 0; g < Gp; g++) {
            const double* ml = pmail + 12 * g;
            if (ml[10] != 0.0) continue;                   // gated: nothing was applied
            const double Si[4] = {ml[4], ml[5], ml[6], ml[7]};
            // (the W rows this correction couples with are the zeta rows of cur's features: this wave's own lanes hold them)
            const double2 w = *reinterpret_cast<const double2*>(Wp + row * BLD + 2 * g);
            const double k0 = fma(w.x, Si[0], w.y * Si[2]), k1 = fma(w.x, Si[1], w.y * Si[3]);
            const double a0 = -La * k0, a1 = -La * k1, b0 = -Lb * k0, b1 = -Lb * k1;
#pragma unroll
            for (int c = 0; c < NC; c += 2) {
              if (c < 2 * Gn) {                            // (uniform)
                const int Lc = 3 * (c >> 1);
                const double wa0 = psv_rl(w.x, Lc), wa1 = psv_rl(w.y, Lc), wb0 = psv_rl(w.x, Lc + 1), wb1 = psv_rl(w.y, Lc + 1);
                sp[c] = psv_sub(sp[c], a0, a1, wa0, wa1);
                sp[c + 1] = psv_sub(sp[c + 1], b0, b1, wb0, wb1);
              }
            }
          }
          __builtin_amdgcn_sched_barrier(0);
          const bool fresh = !in_set(fq, p0, p1, p2);
#pragma unroll 1
          for (int g = 0; g < Gp; g++) {
            const double* ml = pmail + 12 * g;
            if (ml[10] != 0.0) continue;
            const double Si[4] = {ml[4], ml[5], ml[6], ml[7]};
            const double2 w = *reinterpret_cast<const double2*>(Wp + row * BLD + 2 * g);
            const double k0 = fma(w.x, Si[0], w.y * Si[2]), k1 = fma(w.x, Si[1], w.y * Si[3]);
            const double dv = (l * k0) * ml[8] + (l * k1) * ml[9];
            const double kw = Lii * (k0 * w.x + k1 * w.y);
            const double dv1 = __shfl_down(dv, 1), dv2 = __shfl_down(dv, 2), kw2 = __shfl_down(kw, 2);
            if (fresh) {
              double qn[4];
              q_feat_boxplus_fast(sq, dv, dv1, qn);
              sq[0] = qn[0]; sq[1] = qn[1]; sq[2] = qn[2]; sq[3] = qn[3];
              srho += dv2;
              sprr -= kw2;
              fix_depth_v(srho, sprr);
            }
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        if (svalid && sc_l == 0) {
          double* cp = smem + L.cpre + 6 * sq_l;
          cp[0] = sq[0]; cp[1] = sq[1]; cp[2] = sq[2]; cp[3] = sq[3]; cp[4] = srho; cp[5] = sprr;
        }
        PSV_STAMP(7);
        int sbad = 0;
#pragma unroll
        for (int g = 0; g < BG; g++) {                     // (unrolled: the column indices are compile-time, the row stays in registers)
          if (g < Gn) {
            const int wi = gml[g], L0 = 3 * g;
            // prediction, innovation, S^-1, gate of measurement g (:209-239): uniform values from the lanes of feature g
            double qg[4], zhat[2], hb[4];
#pragma unroll
            for (int k = 0; k < 4; k++) qg[k] = psv_rl(sq[k], L0);
            {
              double t1[3], t2[3], zt[3];
              bearing_frame_fast(qg, t1, t2, zt);
              h_feat_frame(t1, t2, zt, prm, zhat, hb);
            }
            const double r0 = wz[2 * wi] - zhat[0], r1 = wz[2 * wi + 1] - zhat[1];
            const double* R = wR + 4 * wi;
            const double p00 = psv_rl(sp[2 * g], L0), p01 = psv_rl(sp[2 * g + 1], L0), p10 = psv_rl(sp[2 * g], L0 + 1), p11 = psv_rl(sp[2 * g + 1], L0 + 1);
            double Si[4];
            const double mahal = feat_innovation(hb, p00, p01, p10, p11, R, r0, r1, Si);   // :230-234
            const bool gate = mahal > kGateMahal;
            if (hb[0] != hb[0] || hb[1] != hb[1] || hb[2] != hb[2] || hb[3] != hb[3]) sbad = 1;
            if (lane == 0) {
              double* ml = mail + 12 * g;
              ml[0] = hb[0]; ml[1] = hb[1]; ml[2] = hb[2]; ml[3] = hb[3];
              ml[4] = Si[0]; ml[5] = Si[1]; ml[6] = Si[2]; ml[7] = Si[3];
              ml[8] = r0; ml[9] = r1; ml[10] = gate ? 1.0 : 0.0; ml[11] = 0.0;
            }
            if (!gate) {                                   // (a gated measurement changes nothing, not even through fix_depth: :235-239)
              double w0, w1, k0, k1;
              psv_wk(sp[2 * g], sp[2 * g + 1], hb, Si, w0, w1, k0, k1);
              if (svalid && (k0 != k0 || k1 != k1)) sbad = 1;
              const double a0 = -La * k0, a1 = -La * k1, b0 = -Lb * k0, b1 = -Lb * k1;
              // the later column pairs of this row, and the couplings for everybody else's rows
#pragma unroll
              for (int gp = g + 1; gp < BG; gp++) {
                if (gp < Gn) {                             // (uniform)
                  const int Lj = 3 * gp;
                  const double wa0 = psv_rl(w0, Lj), wa1 = psv_rl(w1, Lj), wb0 = psv_rl(w0, Lj + 1), wb1 = psv_rl(w1, Lj + 1);
                  sp[2 * gp] = psv_sub(sp[2 * gp], a0, a1, wa0, wa1);
                  sp[2 * gp + 1] = psv_sub(sp[2 * gp + 1], b0, b1, wb0, wb1);
                  if (lane == 0) {
                    double* ct = ctab + 4 * psv_tri(g, gp, BG);
                    *reinterpret_cast<double2*>(ct) = make_double2(wa0, wa1);
                    *reinterpret_cast<double2*>(ct + 2) = make_double2(wb0, wb1);
                  }
                }
              }
              // state correction of the group's features  x <- x [+] (lambda o K r)  (:254-255), rho-rho diagonal, fix_depth (:271)
              const double dv = (l * k0) * r0 + (l * k1) * r1;
              const double kw = Lii * (k0 * w0 + k1 * w1);
              const double dv1 = __shfl_down(dv, 1), dv2 = __shfl_down(dv, 2), kw2 = __shfl_down(kw, 2);
              double qn[4];
              q_feat_boxplus_fast(sq, dv, dv1, qn);
              sq[0] = qn[0]; sq[1] = qn[1]; sq[2] = qn[2]; sq[3] = qn[3];
              srho += dv2;
              sprr -= kw2;
              fix_depth_v(srho, sprr);
            }
          }
        }
        if (sbad) spec[pb] = 1;
        if (svalid && sc_l == 0) {
          double* cb = cbuf + 6 * sq_l;
          cb[0] = sq[0]; cb[1] = sq[1]; cb[2] = sq[2]; cb[3] = sq[3]; cb[4] = srho; cb[5] = sprr;
        }
        __builtin_amdgcn_s_setprio(0);
      }
    } else if (Gp > 0) {
      // ---- D of prev: the features outside prev and cur (prev's are committed, cur's ride with the service wave) and the body,
      //      measurement by measurement from the stored W rows, on the lanes that own them; then prev's pass on these seven waves
      const double* pmail = smem + L.mail + (pb ^ 1) * L.mail_sz;
      if (tid == T - 65) {                                 // (a worker thread without a feature of its own: T - 65 >= N, grouped_choice)
#pragma unroll 1
        for (int g = 0; g < Gp; g++) {
          const double* ml = pmail + 12 * g;
          if (ml[10] != 0.0) continue;
          const double Si[4] = {ml[4], ml[5], ml[6], ml[7]}, r0 = ml[8], r1 = ml[9];
          double dxb[16], xo[17];
#pragma unroll
          for (int q = 0; q < 16; q++) {
            const double lq = partial ? lam[q] : 1.0;
            double q0, q1;
            krow(q, g, Si, q0, q1);
            dxb[q] = (lq * q0) * r0 + (lq * q1) * r1;
          }
          body_boxplus_fast(xs, dxb, xo);
#pragma unroll
          for (int q = 0; q < 17; q++) xs[q] = xo[q];
        }
      }
      for (int f = tid; f < len; f += T - 64) {
        if (in_set(f, p0, p1, p2) || in_set(f, c0, c1, c2)) continue;
        const int d = 16 + 3 * f;
        double* xf = xs + xZ + 5 * f;
        double qf[4] = {xf[0], xf[1], xf[2], xf[3]}, rho = xf[4], prr = diag[f];
        const double l0 = partial ? lam[d] : 1.0, l1 = partial ? lam[d + 1] : 1.0, l2 = partial ? lam[d + 2] : 1.0;
        const double Lii = partial ? (l2 + l2 - l2 * l2) : 1.0;
#pragma unroll 1
        for (int g = 0; g < Gp; g++) {
          const double* ml = pmail + 12 * g;
          if (ml[10] != 0.0) continue;
          const double Si[4] = {ml[4], ml[5], ml[6], ml[7]}, r0 = ml[8], r1 = ml[9];
          double a0, a1, b0, b1, e0, e1;
          krow(d, g, Si, a0, a1); krow(d + 1, g, Si, b0, b1); krow(d + 2, g, Si, e0, e1);
          const double dv0 = (l0 * a0) * r0 + (l0 * a1) * r1, dv1 = (l1 * b0) * r0 + (l1 * b1) * r1, dv2 = (l2 * e0) * r0 + (l2 * e1) * r1;
          double qn[4];
          q_feat_boxplus_fast(qf, dv0, dv1, qn);
          qf[0] = qn[0]; qf[1] = qn[1]; qf[2] = qn[2]; qf[3] = qn[3];
          rho += dv2;
          const double2 wr = *reinterpret_cast<const double2*>(Wp + (d + 2) * BLD + 2 * g);
          prr -= Lii * (e0 * wr.x + e1 * wr.y);
          fix_depth_v(rho, prr);
        }
        xf[0] = qf[0]; xf[1] = qf[1]; xf[2] = qf[2]; xf[3] = qf[3]; xf[4] = rho;
        diag[f] = prr;
      }
      PSV_STAMP(1);
    }
    PSV_STAMP(2);
    // prev's pass over P (psv_pass above); the units are drawn from a counter, so the waves that come late (the three with feature
    // lanes, the one with the body lane, the service wave) take what is left.  (The rho-rho diagonal is kept in LDS: written at the end.)
#ifdef VIEKF_STAMPS
    if (Gp > 0) psv_pass<T, BLD>(P, ld, nact, Gp, Wp, SiL, lam, partial, lane, ticket,
                                 (b == 0 && stamp_iter == 1) ? reinterpret_cast<unsigned long long*>(a.ws) + 128 + 16 * wave : nullptr);
#else
    if (Gp > 0) psv_pass<T, BLD>(P, ld, nact, Gp, Wp, SiL, lam, partial, lane, ticket);
#endif
    PSV_STAMP(6);
    __syncthreads();                                       // prev's pass is done; cur's mail / ctab / cbuf are ready
    PSV_STAMP(3);
    Gp = 0;
    if (Gn == 0) break;
    const double* mail = smem + L.mail + pb * L.mail_sz;
    const double* ctab = smem + L.ctab + pb * L.ctab_sz;
    const int* gsl = reinterpret_cast<const int*>(smem + L.gsl + pb * L.slot_stride);
    const int* gml = gsl + 2 * (L.gml - L.gsl);

    // ================= A: panel <- the zeta columns of cur's features from the lower triangle of P (one row per thread)
    // (all 32 column loads of the row in flight: this phase is four memory latencies long with eight at a time, and nothing else
    //  runs beside it)
    group_load_panel<T, BLD, NC, NC>(P, ld, nact, Gn, gsl, Wp, tid);
    if (tid < 4 * BG) SiL[tid] = 0.0;
    PSV_STAMP(4);

    // ================= C: every row follows on its own (its raw values are its own: no barrier after A); W rows stored; NaN guard
    {
      const int i = tid;                                   // this thread's row of the panel (T >= n: grouped_choice)
      if (i < nact) {
        double rw[NC];
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
          const double2 v = *reinterpret_cast<const double2*>(Wp + i * BLD + c);
          rw[c] = v.x; rw[c + 1] = v.y;
        }
        double La = 1.0, Lb = 1.0;
        if (partial) { const double li = lam[i], la = lam[16], lb = lam[17]; La = la + li - li * la; Lb = lb + li - li * lb; }
        int bad = 0;
#pragma unroll
        for (int g = 0; g < BG; g++) {                     // (unrolled: the row stays in registers under compile-time indices)
          if (g < Gn) {
            const double* ml = mail + 12 * g;
            if (ml[10] != 0.0) {                           // gated: a zero pair (nothing to apply in the pass)
              *reinterpret_cast<double2*>(Wp + i * BLD + 2 * g) = make_double2(0.0, 0.0);
            } else {
              double hb[4], Si[4], w0, w1, k0, k1;
#pragma unroll
              for (int k = 0; k < 4; k++) { hb[k] = ml[k]; Si[k] = ml[4 + k]; }
              psv_wk(rw[2 * g], rw[2 * g + 1], hb, Si, w0, w1, k0, k1);
              if (k0 != k0 || k1 != k1) bad = 1;
              *reinterpret_cast<double2*>(Wp + i * BLD + 2 * g) = make_double2(w0, w1);
              const double a0 = -La * k0, a1 = -La * k1, b0 = -Lb * k0, b1 = -Lb * k1;
#pragma unroll
              for (int gp = g + 1; gp < BG; gp++) {
                if (gp < Gn) {
                  const double* ct = ctab + 4 * psv_tri(g, gp, BG);
                  const double2 wa = *reinterpret_cast<const double2*>(ct), wb = *reinterpret_cast<const double2*>(ct + 2);
                  rw[2 * gp] = psv_sub(rw[2 * gp], a0, a1, wa.x, wa.y);
                  rw[2 * gp + 1] = psv_sub(rw[2 * gp + 1], b0, b1, wb.x, wb.y);
                }
              }
            }
          }
        }
        if (bad) spec[pb] = 1;
      }
    }
    __syncthreads();                                       // W rows complete; the verdict on the speculation
    PSV_STAMP(5);
    const bool failed = spec[pb] != 0;
    if (failed && tid < Gn) {                              // the group's features as they stood BEFORE its chain (the previous group's
      const double* cp = smem + L.cpre + 6 * tid;          // corrections reached them through the service wave only)
      const int fq = gsl[tid];
      double* xf = xs + xZ + 5 * fq;
      xf[0] = cp[0]; xf[1] = cp[1]; xf[2] = cp[2]; xf[3] = cp[3]; xf[4] = cp[4];
      diag[fq] = cp[5];
    }
    if (failed && Gn > 1) {                                // redo these measurements one per group: nothing else has been committed
      single_until = m;
      m = mbase;
      __syncthreads();                                     // (everybody has read the verdict before the flag is cleared)
      form_group();
      continue;
    }
    // ================= commit.  (failed with ONE measurement: the exact NaN-guard verdict -- update skipped, fix_depth runs, :247,271)
    if (tid < Gn) {
      const double* ml = mail + 12 * tid;
      const bool gate = ml[10] != 0.0;
      if (!gate && !failed) group_pack_si(SiL + 4 * tid, ml + 4);
      if (result_all) result_all[(long)b * M + mbase + gml[tid]] = gate ? 1 : 0;
    }
    if (failed) {
      __syncthreads();                                     // (the fall-back state above is in place)
      if (mail[10] == 0.0)
        for (int f = tid; f < len; f += T) { double rho = xs[xZ + 5 * f + 4], prr = diag[f]; fix_depth_v(rho, prr); xs[xZ + 5 * f + 4] = rho; diag[f] = prr; }
      Gp = 0; p0 = 0; p1 = 0; p2 = 0;                      // (no pass: nothing was applied)
    } else {
      if (tid < Gn) {                                      // cur's features: as the service wave left them
        const double* cb = smem + L.cbuf + pb * L.cbuf_sz + 6 * tid;
        const int fq = gsl[tid];
        double* xf = xs + xZ + 5 * fq;
        xf[0] = cb[0]; xf[1] = cb[1]; xf[2] = cb[2]; xf[3] = cb[3]; xf[4] = cb[4];
        diag[fq] = cb[5];
      }
      Gp = Gn; p0 = c0; p1 = c1; p2 = c2;
    }
    // ================= the next group; the service wave reads its entries of P before the pass of the group just committed starts
    pb ^= 1;
    form_group();                                          // (its barriers also publish the commit above)
  }
  // ---- the launch's last words: state, rho-rho diagonal, flags
  for (int f = tid; f < len; f += T) P[(16 + 3 * f + 2) + (long)(16 + 3 * f + 2) * ld] = diag[f];
  group_store_state<T>(xs, xg, len, tid, flag, &a.flags[b]);
}

}  // namespace viekf
