// viekf_kernels_stream.hpp -- "streaming" kernel family: one workgroup per filter, covariance stays
// in HBM/L2 (column-major, leading dimension ld) and is updated in place.  Works for any number of
// features; it is the path for wide P (N=150) and the correctness baseline for the resident family.
//
// Structure exploited (exact in real arithmetic):
//   A = [[A_bb, 0], [A_fb, blockdiag(A_ff)]]   (vi_ekf_dyn.cpp:55-71,121-128: body rows never depend on features)
//   => Phi = I + A dt + A^2 dt^2/2 has the same shape, so  P+ = Phi P Phi^T + Gd Qu Gd^T + Qx  (vi_ekf.cpp:302-304)
//      needs per 3x3 block only its own block plus the 16 body rows/columns.
//   H of a FEAT measurement has one 2x2 block (vi_ekf_meas.cpp:366) => W = P H^T is two columns of P and
//      (I-KH)P(I-KH)^T + KRK^T - P = -K W^T, so the partial update (vi_ekf_meas.cpp:254-257) is
//      P_ij -= Lambda_ij (K_i . W_j),  Lambda_ij = l_i + l_j - l_i l_j  (vi_ekf.cpp:83,146).
//
// Defines kernels: included from viekf_dispatch.hpp only.  The kernel arguments are viekf_kernel_args.hpp, the dynamic-LDS
// carve-ups of k_propagate_stream and k_update_feat_stream viekf_stream_lds.hpp (BlkLds, the grouped update's, is below).
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_onepass.hpp"
#include "viekf_stream_lds.hpp"

namespace viekf {

// ------------------------------------------------------------------------------------------------
// propagate: numeric core of VIEKF::propagate_state (vi_ekf.cpp:262-318)
// ------------------------------------------------------------------------------------------------
// MF = true: the feature/feature part runs on the fp64 matrix cores (see the pass at the end); otherwise one 3x3 block per thread.
template <int T, bool MF>
__global__ __launch_bounds__(T) void k_propagate_stream(StreamArgs a, const double* __restrict__ u_all,
                                                        const double* __restrict__ dt_all) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  if (a.active && !a.active[b]) return;
  const int n = a.n, ld = a.ld;
  const PropLds lds(a.nxs, sizeof(BodyCtx), a.N, MF);
  double* xs = smem + lds.xs;           // [nxs]
  double* Abb = smem + lds.Abb;         // 16x16 row-major
  double* Gb = smem + lds.Gb;           // 16x6
  double* Phibb = smem + lds.Phibb;     // 16x16
  double* Mbb = smem + lds.Mbb;         // 16x16
  double* Gdb = smem + lds.Gdb;         // 16x6
  double* Pbb = smem + lds.Pbb;         // 16x16 row-major copy of P_bb
  double* T16 = smem + lds.T16;         // 16x16 scratch
  double* xdb = smem + lds.xdb;         // 16
  BodyCtx* ctx = reinterpret_cast<BodyCtx*>(smem + lds.ctx);
  double* Dl = smem + lds.Dl;           // [N][9] Phi_ff blocks (MF only)

  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nf = 3 * len, nact = 16 + nf;
  const double dt = dt_all[b];
  const WsLayout L(a.N, n);
  double* ws = a.ws + (long)b * a.ws_stride;
  double* phi_fb = ws + L.phi_fb;
  double* phi_ff = ws + L.phi_ff;
  double* gd = ws + L.gd;
  double* U = ws + L.U;
  double* pbr = ws + L.pbr;
  double* pbc = ws + L.pbc;

  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  __syncthreads();

  if (tid == 0) {
    double ub[6];
    q_rota(a.prm(b).q_b_u, u_all + (long)b * 6, ub);          // vi_ekf.cpp:265-267
    q_rota(a.prm(b).q_b_u, u_all + (long)b * 6 + 3, ub + 3);
    body_ctx(xs, ub, a.prm(b), *ctx);
    body_dynamics(*ctx, a.prm(b), xdb, Abb, Gb);               // vi_ekf_dyn.cpp:42-80
  }
  __syncthreads();

  // ---- body transition blocks (vi_ekf.cpp:302-303 restricted to the 16x16 block)
  for (int e = tid; e < 256; e += T) {
    const int r = e >> 4, c = e & 15;
    double a2 = 0.0;
    for (int k = 0; k < 16; k++) a2 += Abb[r * 16 + k] * Abb[k * 16 + c];
    const double id = (r == c) ? 1.0 : 0.0, av = Abb[e];
    Mbb[e] = id + av * dt / 2.0 + a2 * dt * dt / 6.0;
    Phibb[e] = id + av * dt + a2 * dt * dt / 2.0;
  }
  __syncthreads();
  for (int e = tid; e < 96; e += T) {
    const int r = e / 6, k = e % 6;
    double s = 0.0;
    for (int c = 0; c < 16; c++) s += Mbb[r * 16 + c] * Gb[c * 6 + k];
    s *= dt;
    Gdb[e] = s;
    gd[r * 6 + k] = s;
  }

  // ---- per feature: dynamics, Phi_fb / Phi_ff / Gd_f, state step
  for (int i = tid; i < len; i += T) {
    double xd3[3], Afv[9], Afg[9], Aff[9];
    const double* qz = xs + xZ + 5 * i;
    const double rho = qz[4];
    feature_dynamics(qz, rho, *ctx, xd3, Afv, Afg, Aff);   // vi_ekf_dyn.cpp:96-134
    double Aff2[9];
    mm<3, 3, 3>(Aff, Aff, Aff2);
    double Mff[9];
    for (int e = 0; e < 9; e++) {
      const double id = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
      Mff[e] = id + Aff[e] * dt / 2.0 + Aff2[e] * dt * dt / 6.0;
      const double ph = id + Aff[e] * dt + Aff2[e] * dt * dt / 2.0;
      phi_ff[9 * i + e] = ph;
      if (MF) Dl[9 * i + e] = ph;
    }
    double gacc[18];
    for (int e = 0; e < 18; e++) gacc[e] = 0.0;
#pragma unroll
    for (int c = 0; c < 16; c++) {
#pragma unroll
      for (int r = 0; r < 3; r++) {
        // A_fb(r,c): non-zero only in the VEL and B_G columns
        double afb = 0.0;
        if (c >= dxVEL && c < dxVEL + 3) afb = Afv[r * 3 + (c - dxVEL)];
        else if (c >= dxB_G && c < dxB_G + 3) afb = Afg[r * 3 + (c - dxB_G)];
        // (A^2)_fb = A_fb A_bb + A_ff A_fb
        double a2 = 0.0;
        for (int k = 0; k < 3; k++) a2 += Afv[r * 3 + k] * Abb[(dxVEL + k) * 16 + c] + Afg[r * 3 + k] * Abb[(dxB_G + k) * 16 + c];
        if (c >= dxVEL && c < dxVEL + 3)
          for (int k = 0; k < 3; k++) a2 += Aff[r * 3 + k] * Afv[k * 3 + (c - dxVEL)];
        else if (c >= dxB_G && c < dxB_G + 3)
          for (int k = 0; k < 3; k++) a2 += Aff[r * 3 + k] * Afg[k * 3 + (c - dxB_G)];
        phi_fb[(3 * i + r) * 16 + c] = afb * dt + a2 * dt * dt / 2.0;
        const double mfb = afb * dt / 2.0 + a2 * dt * dt / 6.0;
        for (int k = 0; k < 6; k++) gacc[r * 6 + k] += mfb * Gb[c * 6 + k];
      }
    }
    for (int r = 0; r < 3; r++)
      for (int k = 0; k < 3; k++) {   // G_f = [0 | Afg]  (vi_ekf_dyn.cpp:131-132)
        double s = 0.0;
        for (int m = 0; m < 3; m++) s += Mff[r * 3 + m] * Afg[m * 3 + k];
        gacc[r * 6 + 3 + k] += s;
      }
    for (int e = 0; e < 18; e++) gd[(16 + 3 * i) * 6 + e] = gacc[e] * dt;
    // state step for this feature (boxplus, vi_ekf_helper.cpp:93-97)
    double qn[4];
    q_feat_boxplus(qz, xd3[0] * dt, xd3[1] * dt, qn);
    xs[xZ + 5 * i + 0] = qn[0]; xs[xZ + 5 * i + 1] = qn[1]; xs[xZ + 5 * i + 2] = qn[2]; xs[xZ + 5 * i + 3] = qn[3];
    xs[xZ + 5 * i + 4] = rho + xd3[2] * dt;
  }
  // ---- save the body rows / columns of P before anything is overwritten
  // (the matrix-core variant reads nothing above the diagonal outside the diagonal 48 x 48 super-tiles: after a grouped update
  //  the rest of the upper triangle may be stale, see k_update_feat_blocked; P is symmetric, so the body rows are the body columns)
  for (int e = tid; e < 16 * nact; e += T) {
    const int k = e / nact, j = e % nact;
    const double pc = P[j + (long)k * ld];
    pbr[k * n + j] = MF ? pc : P[k + (long)j * ld];
    pbc[k * n + j] = pc;
  }
  for (int e = tid; e < 256; e += T) Pbb[e] = MF ? P[max(e >> 4, e & 15) + (long)min(e >> 4, e & 15) * ld] : P[(e >> 4) + (long)(e & 15) * ld];
  __syncthreads();
  if (tid == 0) {  // body state step (after every feature thread has read the old body state through ctx)
    double dxb[16], xo[17];
    for (int i = 0; i < 16; i++) dxb[i] = xdb[i] * dt;
    body_boxplus(xs, dxb, xo);
    for (int i = 0; i < 17; i++) xs[i] = xo[i];
  }

  // ---- U = (Phi P)[feat, body]  (its mirror (P Phi^T)[body, feat] is not formed: P+ is written symmetric),  T16 = Phi_bb P_bb
  for (int e = tid; e < nf * 16; e += T) {
    const int r = e >> 4, k = e & 15, I = r / 3, rr = r - 3 * I;
    double s = 0.0;
    for (int c = 0; c < 16; c++) s += phi_fb[r * 16 + c] * Pbb[c * 16 + k];
    double vt = 0.0;
    for (int m = 0; m < 3; m++) {
      const double pf = phi_ff[9 * I + rr * 3 + m];
      s += pf * pbc[k * n + 16 + 3 * I + m];
      vt += pbr[k * n + 16 + 3 * I + m] * pf;
    }
    U[r * 16 + k] = s;
    if (MF) {
      // rows of the low-rank factors:  P+_ff - D P_ff D^T = U Phi_fb^T + Phi_fb (P_bf D^T) + (Gd Qu) Gd^T = Xw Yw^T
      double* xr = ws + L.Xw + (long)r * WK;
      double* yr = ws + L.Yw + (long)r * WK;
      const double ph = phi_fb[r * 16 + k];
      xr[k] = s;       yr[k] = ph;
      xr[16 + k] = ph; yr[16 + k] = vt;
      if (k < 8) {
        const double g = (k < 6) ? gd[(16 + r) * 6 + k] : 0.0;
        xr[32 + k] = (k < 6) ? g * a.prm(b).Qu[k] : 0.0;
        yr[32 + k] = g;
      }
    }
  }
  for (int e = tid; e < 256; e += T) {
    const int r = e >> 4, c = e & 15;
    double s = 0.0;
    for (int k = 0; k < 16; k++) s += Phibb[r * 16 + k] * Pbb[k * 16 + c];
    T16[e] = s;
  }
  __syncthreads();

  // ---- write P+ : body block
  // P+ is written EXACTLY symmetric (every pair gets one value): the update kernels' rank-2 form equals the reference's
  // Joseph form only for symmetric P and amplifies an antisymmetric part instead of damping it (see the fused kernel's
  // sym_diag), so rounding-level asymmetry must not be allowed to build up over a flight.
  for (int e = tid; e < 256; e += T) {
    const int r = min(e >> 4, e & 15), c = max(e >> 4, e & 15);   // the (lower index, higher index) expression for both copies
    double s = 0.0;
    for (int k = 0; k < 16; k++) s += T16[r * 16 + k] * Phibb[c * 16 + k];
    double g = 0.0;
    for (int k = 0; k < 6; k++) g += Gdb[r * 6 + k] * a.prm(b).Qu[k] * Gdb[c * 6 + k];
    s = s + g;
    if (r == c) s += a.qx(b)[r];
    P[(e >> 4) + (long)(e & 15) * ld] = s;
  }
  // ---- body/feature cross blocks (the feature-row copy, mirrored)
  for (int e = tid; e < nf * 16; e += T) {
    const int r = e >> 4, k = e & 15;
    double s = 0.0;
    for (int c = 0; c < 16; c++) s += U[r * 16 + c] * Phibb[k * 16 + c];
    double g = 0.0;
    for (int q = 0; q < 6; q++) g += gd[(16 + r) * 6 + q] * a.prm(b).Qu[q] * Gdb[k * 6 + q];
    P[(16 + r) + (long)k * ld] = s + g;
    if (!MF) P[k + (long)(16 + r) * ld] = s + g;   // (the matrix-core variant keeps the lower triangle only, see below)
  }
  if constexpr (MF) {
    // ---- feature/feature part on the matrix cores.  With D = blockdiag(Phi_ff) the new block is
    //        P+_ff = D P_ff D^T + Xw Yw^T          (Xw, Yw: nf x 38, rows written above)
    //      One wave per 48 x 48 super-tile (16 features square, so D never straddles a tile), v_mfma_f64_16x16x4_f64:
    //        R   = P_IJ D_J^T              A = P (lane & 15 along the rows of P: coalesced loads), B = D_J^T built from LDS
    //        O^T = R^T D_I^T               A = R straight from the accumulators: register s of a 16x16 result IS the operand of
    //                                      k-step s (row (lane>>4) + 4 s), so the chain needs no data movement
    //        O^T += Yw_J Xw_I^T            10 k-steps
    //      O^T has lane & 15 along the rows of P again: coalesced stores.  D is block-diagonal, so only the k-steps that
    //      overlap a tile's features are issued (16 of 36 per product).  In place: a super-tile depends on itself only.
    __syncthreads();   // Xw / Yw rows and Dl are complete (this block's global writes are visible to it after the barrier)
    const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
    constexpr int NWV = T / 64;
    const int nst = (nf + 47) / 48;
    const double* Xw = ws + L.Xw;
    const double* Yw = ws + L.Yw;
    // operand element D[16 q + lr][4 s + lk] of the 48 x 48 block-diagonal matrix of super-tile `sup`
    auto dop = [&](int sup, int q, int s) -> double {
      const int jp = 16 * q + lr, j = 4 * s + lk;
      const int fp = jp / 3, f = j / 3, F = 16 * sup + fp;
      return (fp == f && F < len) ? Dl[9 * F + (jp - 3 * fp) * 3 + (j - 3 * f)] : 0.0;
    };
    // Only the super-tiles on and below the diagonal are computed and only the elements i >= j stored: the hot kernels (this one,
    // the grouped update, the fused step) read the LOWER triangle of P only, so nothing above the diagonal is written here --
    // r02's transpose pass cost one more read and one more write of half the matrix per step.  The host marks the batch
    // (upper_stale) and mirrors the triangle up (k_mirror_upper) before anything reads P whole.
    for (int st = wave; st < nst * nst; st += NWV) {
      const int I = st % nst, J = st / nst;
      if (I < J) continue;
      const int r0 = 16 + 48 * I, c0 = 16 + 48 * J;
      double pA[3][12];
#pragma unroll
      for (int aa = 0; aa < 3; aa++)
#pragma unroll
        for (int s = 0; s < 12; s++)
        {   // (a diagonal super-tile: the elements above the diagonal through their mirrors -- only the lower triangle is valid)
          const int pi = min(r0 + 16 * aa + lr, nact - 1), pj = min(c0 + 4 * s + lk, nact - 1);
          pA[aa][s] = P[max(pi, pj) + (long)min(pi, pj) * ld];
        }
      v4f64 R[3][3], O[3][3];
#pragma unroll
      for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int aa = 0; aa < 3; aa++) { R[aa][q] = v4f64{0.0, 0.0, 0.0, 0.0}; O[q][aa] = v4f64{0.0, 0.0, 0.0, 0.0}; }
      }
#pragma unroll
      for (int q = 0; q < 3; q++) {
        constexpr int S0[3] = {0, 3, 7}, S1[3] = {4, 8, 11};   // k-steps (4 columns each) that touch the features of tile q
#pragma unroll
        for (int s = 0; s < 12; s++) {
          if (s < S0[q] || s > S1[q]) continue;
          const double bd = dop(J, q, s);
#pragma unroll
          for (int aa = 0; aa < 3; aa++) R[aa][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(pA[aa][s], bd, R[aa][q], 0, 0, 0);
        }
      }
#pragma unroll
      for (int aa = 0; aa < 3; aa++) {
        constexpr int S0[3] = {0, 3, 7}, S1[3] = {4, 8, 11};
#pragma unroll
        for (int s = 0; s < 12; s++) {
          if (s < S0[aa] || s > S1[aa]) continue;
          const double bi = dop(I, aa, s);
#pragma unroll
          for (int q = 0; q < 3; q++) O[q][aa] = __builtin_amdgcn_mfma_f64_16x16x4f64(R[s / 4][q][s % 4], bi, O[q][aa], 0, 0, 0);
        }
      }
#pragma unroll 2
      for (int s = 0; s < WK / 4; s++) {
        double yv[3], xv[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
          yv[q] = Yw[(long)(48 * J + 16 * q + lr) * WK + 4 * s + lk];
          xv[q] = Xw[(long)(48 * I + 16 * q + lr) * WK + 4 * s + lk];
        }
#pragma unroll
        for (int q = 0; q < 3; q++)
#pragma unroll
          for (int aa = 0; aa < 3; aa++) O[q][aa] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv[q], xv[aa], O[q][aa], 0, 0, 0);
      }
#pragma unroll
      for (int q = 0; q < 3; q++)
#pragma unroll
        for (int aa = 0; aa < 3; aa++) {
          const int i = r0 + 16 * aa + lr;
#pragma unroll
          for (int rg = 0; rg < 4; rg++) {
            const int j = c0 + 16 * q + lk + 4 * rg;
            if (i < nact && j < nact && i >= j) {
              double v = O[q][aa][rg];
              if (i == j) v += a.qx(b)[i];
              P[i + (long)j * ld] = v;
            }
          }
        }
    }
  } else {
    // ---- feature/feature 3x3 blocks, in place (each block needs only itself + saved body strips)
    for (int e = tid; e < len * len; e += T) {
      const int I = e % len, J = e / len;
      if (I < J) continue;                       // (the block below the diagonal is computed, its mirror written with it)
      const int r0 = 16 + 3 * I, c0 = 16 + 3 * J;
      double Pij[9], Mij[9], out[9];
      for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) Pij[r * 3 + c] = P[(r0 + r) + (long)(c0 + c) * ld];
      for (int r = 0; r < 3; r++)
        for (int m = 0; m < 3; m++) {
          double s = 0.0;
          for (int k = 0; k < 16; k++) s += phi_fb[(3 * I + r) * 16 + k] * pbr[k * n + c0 + m];
          for (int q = 0; q < 3; q++) s += phi_ff[9 * I + r * 3 + q] * Pij[q * 3 + m];
          Mij[r * 3 + m] = s;
        }
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
          double s = 0.0;
          for (int k = 0; k < 16; k++) s += U[(3 * I + r) * 16 + k] * phi_fb[(3 * J + c) * 16 + k];
          for (int m = 0; m < 3; m++) s += Mij[r * 3 + m] * phi_ff[9 * J + c * 3 + m];
          double g = 0.0;
          for (int q = 0; q < 6; q++) g += gd[(r0 + r) * 6 + q] * a.prm(b).Qu[q] * gd[(c0 + c) * 6 + q];
          s = s + g;
          if (I == J && r == c) s += a.qx(b)[r0 + r];
          out[r * 3 + c] = s;
        }
      if (I == J) { out[1] = out[3]; out[2] = out[6]; out[5] = out[7]; }   // diagonal block: upper <- lower
      for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) {
          P[(r0 + r) + (long)(c0 + c) * ld] = out[r * 3 + c];
          if (I != J) P[(c0 + c) + (long)(r0 + r) * ld] = out[r * 3 + c];
        }
    }
  }
  // inactive slots: Phi = I and G = 0 there, so only Qx is added (vi_ekf.cpp:139-144,304)
  for (int d = nact + tid; d < n; d += T) P[d + (long)d * ld] += a.qx(b)[d];
  __syncthreads();

  // ---- fix_depth (vi_ekf.cpp:311) and write the state back
  unsigned flag = 0;
  for (int i = tid; i < len; i += T) fix_depth_one(xs, P, ld, i, a.prm(b), flag);
  __syncthreads();
  for (int i = tid; i < xZ + 5 * len; i += T) {
    const double v = xs[i];
    if (v != v) flag |= FLAG_NAN;
    if (v > 1e6) flag |= FLAG_BLOWUP;
    xg[i] = v;
  }
  if (flag) atomicOr(&a.flags[b], flag);
}

// ------------------------------------------------------------------------------------------------
// M sequential active FEAT updates: VIEKF::update + h_feat (vi_ekf_meas.cpp:196-278, 354-367)
// The reference-order baseline the tests compare the other update kernels with: it deliberately keeps h_feat, the LU inv2 and
// W from LDS written out here instead of the fast forms (h_feat_frame, feat_innovation) the other families share.
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_update_feat_stream(StreamArgs a, const double* __restrict__ z_all,
                                                          const int* __restrict__ slot_all, int M,
                                                          const double* __restrict__ R_all, long r_stride_b,
                                                          long r_stride_m, int* __restrict__ result_all) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  if (a.active && !a.active[b]) return;
  const int n = a.n, ld = a.ld;
  const UpdLds lds(a.nxs, n);
  double* xs = smem + lds.xs;     // [nxs]
  double* W = smem + lds.W;       // [n][2]
  double* K = smem + lds.K;       // [n][2]
  double* lam = smem + lds.lam;   // [n]
  double* sm = smem + lds.sm;     // small scratch: zhat(2) Hb(4) res(2) Sinv(4) = 12, dxb(16)
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  unsigned flag = 0;

  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lam(b)[i];
  __syncthreads();

  for (int m = 0; m < M; m++) {
    const int slot = slot_all[(long)b * M + m];
    int* res = result_all ? &result_all[(long)b * M + m] : nullptr;
    if (slot < 0) { if (res && tid == 0) *res = -1; continue; }
    if (slot >= len) { if (res && tid == 0) *res = 3; continue; }  // MEAS_INVALID
    const double* z = z_all + ((long)b * M + m) * 2;
    const double* R = R_all + (long)b * r_stride_b + (long)m * r_stride_m;  // column-major 2x2
    const double z0 = z[0], z1 = z[1];
    if (z0 != z0 || z1 != z1) { if (res && tid == 0) *res = 2; continue; }  // MEAS_NAN (vi_ekf_meas.cpp:136-137)
    const int j0 = 16 + 3 * slot;
    if (tid == 0) {
      double zhat[2], Hb[4];
      h_feat(xs + xZ + 5 * slot, a.prm(b), zhat, Hb);
      sm[0] = zhat[0]; sm[1] = zhat[1];
      sm[2] = Hb[0]; sm[3] = Hb[1]; sm[4] = Hb[2]; sm[5] = Hb[3];
      sm[6] = z0 - zhat[0]; sm[7] = z1 - zhat[1];      // residual (vi_ekf_meas.cpp:220)
    }
    __syncthreads();
    const double h00 = sm[2], h01 = sm[3], h10 = sm[4], h11 = sm[5];
    // W = P H^T : two columns of P (coalesced along i)
    for (int i = tid; i < nact; i += T) {
      const double p0 = P[i + (long)j0 * ld], p1 = P[i + (long)(j0 + 1) * ld];
      W[2 * i + 0] = p0 * h00 + p1 * h01;
      W[2 * i + 1] = p0 * h10 + p1 * h11;
    }
    __syncthreads();
    // S = H W[j0:j0+2] + R ; every lane computes it (uniform)
    double S[4], Si[4];
    {
      const double w00 = W[2 * j0 + 0], w01 = W[2 * j0 + 1], w10 = W[2 * (j0 + 1) + 0], w11 = W[2 * (j0 + 1) + 1];
      S[0] = h00 * w00 + h01 * w10 + R[0];
      S[1] = h00 * w01 + h01 * w11 + R[2];
      S[2] = h10 * w00 + h11 * w10 + R[1];
      S[3] = h10 * w01 + h11 * w11 + R[3];
    }
    inv2(S, Si);
    const double r0 = sm[6], r1 = sm[7];
    const double mahal = (r0 * Si[0] + r1 * Si[2]) * r0 + (r0 * Si[1] + r1 * Si[3]) * r1;  // vi_ekf_meas.cpp:234
    if (mahal > kGateMahal) {                                   // gate (:235-239): returns before fix_depth
      if (res && tid == 0) *res = 1;
      __syncthreads();
      continue;
    }
    // K = W S^-1 (:241) and NaN guard (:247)
    int bad = 0;
    for (int i = tid; i < nact; i += T) {
      const double w0 = W[2 * i], w1 = W[2 * i + 1];
      const double k0 = w0 * Si[0] + w1 * Si[2], k1 = w0 * Si[1] + w1 * Si[3];
      K[2 * i] = k0; K[2 * i + 1] = k1;
      if (k0 != k0 || k1 != k1) bad = 1;
    }
    if (h00 != h00 || h01 != h01 || h10 != h10 || h11 != h11) bad = 1;
    bad = __syncthreads_or(bad);
    if (!bad) {
      const bool partial = a.prm(b).use_partial_update != 0;
      // state correction  x <- x [+] (lambda o K r)   (:254-255 / :262-263)
      if (tid == 0) {
        double dxb[16], xo[17];
        for (int i = 0; i < 16; i++) {
          const double l = partial ? lam[i] : 1.0;
          dxb[i] = (l * K[2 * i]) * r0 + (l * K[2 * i + 1]) * r1;
        }
        body_boxplus(xs, dxb, xo);
        for (int i = 0; i < 17; i++) xs[i] = xo[i];
      }
      for (int f = tid; f < len; f += T) {
        const int d = 16 + 3 * f;
        double dv[3];
        for (int q = 0; q < 3; q++) {
          const double l = partial ? lam[d + q] : 1.0;
          dv[q] = (l * K[2 * (d + q)]) * r0 + (l * K[2 * (d + q) + 1]) * r1;
        }
        double qn[4];
        q_feat_boxplus(xs + xZ + 5 * f, dv[0], dv[1], qn);
        double* xf = xs + xZ + 5 * f;
        xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
        xf[4] += dv[2];
      }
      // covariance sweep  P_ij -= Lambda_ij (K_i . W_j)   (:256-257, or :264-265 with Lambda = 1)
      const long tot = (long)nact * nact;
      for (long e = tid; e < tot; e += T) {
        const int i = (int)(e % nact), j = (int)(e / nact);
        // (i, j) and (j, i) both form K_hi . W_lo from their own, equal, copies: P stays EXACTLY symmetric (this rank-2 form
        //  equals the reference's Joseph form only for symmetric P, and it amplifies an antisymmetric part -- see the fused
        //  kernel's sym_diag)
        const int hi = max(i, j), lo = min(i, j);
        const double t = K[2 * hi] * W[2 * lo] + K[2 * hi + 1] * W[2 * lo + 1];
        const double li = lam[i], lj = lam[j];
        const double L = partial ? (lj + li - li * lj) : 1.0;
        P[i + (long)j * ld] -= L * t;
      }
    }
    __syncthreads();
    for (int f = tid; f < len; f += T) fix_depth_one(xs, P, ld, f, a.prm(b), flag);   // :271
    if (res && tid == 0) *res = 0;
    __syncthreads();
  }
  for (int i = tid; i < xZ + 5 * len; i += T) {
    const double v = xs[i];
    if (v != v) flag |= FLAG_NAN;
    if (v > 1e6) flag |= FLAG_BLOWUP;
    xg[i] = v;
  }
  if (flag) atomicOr(&a.flags[b], flag);
}

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
// (shared by the two grouped update kernels: k_update_feat_blocked below and k_update_feat_panelsvc in viekf_kernels_wide.hpp)
// ticket != NULL: the units are drawn from a counter in LDS instead of being dealt round-robin (waves that arrive late -- they had
// other work first -- then simply take fewer)
template <int T, int BLD>
__device__ __forceinline__ void blk_pass(double* __restrict__ P, int ld, int nact, int Gn, const double* Wp, const double* SiL,
                                         const double* lam, const double* diag, bool partial, int lane, int wave, int* ticket = nullptr) {
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
    auto draw = [&]() {                                  // the unit of the next ticket (wave-uniform)
      int t = 0;
      if (lane == 0) t = atomicAdd(ticket, 1);
      return next_unit(Unit{0, 0}, __builtin_amdgcn_readfirstlane(t));
    };
    double pv[TPI][4];
    Unit u = ticket ? draw() : next_unit(Unit{0, 0}, wave);
    while (u.tj < nt) {
      load_tiles(u, pv);                // (the SIMD's other wave computes meanwhile; an explicit prefetch of the next unit
      const Unit un = ticket ? draw() : next_unit(u, NWV);   //  did not pay for its registers)
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
// BG = measurements per group (template parameter: 16, 24 or 32 -- the largest whose panel fits the LDS, so that the narrower
// filters of this family cross HBM fewer times); BLD = 2 BG + 2 = LDS row stride (doubles) of the n x 2 BG panel; BWIN = 2 BG
// measurement-list entries staged per group

struct BlkLds {
  int xs, lam, Wp, Si, sm, diag, gsl, win, total;   // offsets in doubles
  __host__ __device__ BlkLds(int N, int n, int nxs, int BG) {
    const int nr = (n + 15) & ~15, BLD = 2 * BG + 2, BWIN = 2 * BG;
    int o = 0;
    auto take = [&](int c) { int r = o; o += (c + 1) & ~1; return r; };
    xs = take(nxs); lam = take(n); Wp = take(nr * BLD); Si = take(4 * BG); sm = take(32);   // sm: pzz[2][4] (+ spare)
    diag = take(N > 0 ? N : 1);
    gsl = take(2 * BG);   // ints: slot[BG], measurement index[BG]
    win = take(7 * BWIN);   // staged window of the measurement list: z [BWIN][2], R [BWIN][4], slot [BWIN] (ints)
    total = o;
  }
};

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
  double* pzz = smem + L.sm;    // [2][4] zeta-zeta block of the current / next measurement
  int* badf = reinterpret_cast<int*>(pzz + 8);   // [BG] NaN-guard verdict of each measurement of the group (set by any thread)
  double* diag = smem + L.diag; // running P(rho_f, rho_f)
  int* gsl = reinterpret_cast<int*>(smem + L.gsl);
  int* gml = gsl + BG;
  double* wz = smem + L.win;
  double* wR = wz + 2 * BWIN;
  int* wsl = reinterpret_cast<int*>(wR + 4 * BWIN);
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
    // ---- stage a window of the measurement list in LDS (one parallel fetch instead of a chain of dependent global loads),
    //      then form the next group from it (every thread scans the same list: uniform control flow; tid 0 records it)
    __syncthreads();   // (the previous group is done with the window)
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
    __syncthreads();
    int Gn = 0;
    {
      int mm = m;
      const int mend = min(M, m + BWIN);
      unsigned long long seen0 = 0, seen1 = 0, seen2 = 0;   // slots already in the group (3 x 64 >= the 160-feature limit)
      while (mm < mend && Gn < BG) {
        const int slot = wsl[mm - m];
        if (slot >= 0) {
          unsigned long long& w = slot < 64 ? seen0 : (slot < 128 ? seen1 : seen2);
          const unsigned long long bit = 1ull << (slot & 63);
          if (w & bit) break;                             // repeated slot: it opens the next group
          w |= bit;
          if (tid == 0) { gsl[Gn] = slot; gml[Gn] = mm - m; }   // (index into the window)
          Gn++;
        }
        mm++;
      }
      const int m0 = m;
      m = mm;
      mbase = m0;
    }
    if (Gn == 0) continue;
    // ---- 1. panel <- the zeta columns of the group's features; unused columns <- 0.  Only the LOWER triangle of P is valid:
    //      element (i, c) of a column comes from the column where i >= c (coalesced along the rows) and from ROW c where i < c
    //      (one 8-byte read per thread, a column apart; the rows of a group's features are mostly neighbours -- measurements
    //      arrive in slot order -- so a thread's reads share 128-byte lines).  That costs about a quarter of a pass in fetched
    //      lines per group and saves the mirrored stores of every pass (r02: up to the whole upper triangle per pass, the
    //      kernel's largest single write stream) and the propagate's transpose pass.
    for (int i = tid; i < nact; i += T) {
#pragma unroll 1
      for (int c0 = 0; c0 < 2 * BG; c0 += 8) {           // eight independent column loads in flight per thread
        double v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const int c = c0 + k;
          const int col = 16 + 3 * gsl[(c < 2 * Gn) ? (c >> 1) : 0] + (c & 1);
          v[k] = (c < 2 * Gn) ? P[max(i, col) + (long)min(i, col) * ld] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < 8; k += 2) *reinterpret_cast<double2*>(Wp + i * BLD + c0 + k) = make_double2(v[k], v[k + 1]);
      }
    }
    if (tid < 4 * BG) SiL[tid] = 0.0;
    if (tid < BG) badf[tid] = 0;
    for (int f = tid; f < len; f += T) diag[f] = P[(16 + 3 * f + 2) + (long)(16 + 3 * f + 2) * ld];
    // The zeta-zeta 2x2 of the measurement about to be processed is handed over in pzz[parity][4] by the two threads that own
    // its rows (they are the ones that keep those panel entries current), so nobody reads panel rows that are being rewritten.
    const int i = tid;                                      // this thread's row of the panel (T >= n, checked on the host)
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
        if (tid == 0) { SiL[4 * g + 0] = Si[0]; SiL[4 * g + 1] = Si[2]; SiL[4 * g + 2] = Si[1]; SiL[4 * g + 3] = Si[3]; }
        // state correction  x <- x [+] (lambda o K r)   (:254-255 / :262-263);  K rows re-formed from W where needed
        auto krow = [&](int row, double& q0, double& q1) {
          const double2 w = *reinterpret_cast<const double2*>(Wp + row * BLD + 2 * g);
          q0 = w.x * Si[0] + w.y * Si[2]; q1 = w.x * Si[1] + w.y * Si[3];
        };
        if (tid == T - 1) {                                // (a thread without a feature of its own: T - 1 >= n > len)
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
  for (int i = tid; i < xZ + 5 * len; i += T) {
    const double v = xs[i];
    if (v != v) flag |= FLAG_NAN;
    if (v > 1e6) flag |= FLAG_BLOWUP;
    xg[i] = v;
  }
  if (flag) atomicOr(&a.flags[b], flag);
}

}  // namespace viekf
