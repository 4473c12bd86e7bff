// viekf_kernels_stream.hpp -- "streaming" kernel family: one workgroup per filter, covariance stays
// in HBM/L2 (column-major, leading dimension ld) and is updated in place.  Works for any number of
// features; it is the reference-order baseline of every other family (wide P runs on viekf_kernels_wide.hpp / _grouped.hpp).
//
// Structure exploited (exact in real arithmetic):
//   A = [[A_bb, 0], [A_fb, blockdiag(A_ff)]]   (vi_ekf_dyn.cpp:55-71,121-128: body rows never depend on features)
//   => Phi = I + A dt + A^2 dt^2/2 has the same shape, so  P+ = Phi P Phi^T + Gd Qu Gd^T + Qx  (vi_ekf.cpp:302-304)
//      needs per 3x3 block only its own block plus the 16 body rows/columns.
//   H of a FEAT measurement has one 2x2 block (vi_ekf_meas.cpp:366) => W = P H^T is two columns of P and
//      (I-KH)P(I-KH)^T + KRK^T - P = -K W^T, so the partial update (vi_ekf_meas.cpp:254-257) is
//      P_ij -= Lambda_ij (K_i . W_j),  Lambda_ij = l_i + l_j - l_i l_j  (vi_ekf.cpp:83,146).
//
// Defines k_propagate_stream and k_update_feat_stream and nothing else: included from viekf_dispatch.hpp only.  The kernel
// arguments are viekf_kernel_args.hpp, the dynamic-LDS carve-ups viekf_stream_lds.hpp.  The grouped updates that wide P runs on
// are in viekf_kernels_grouped.hpp.
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

}  // namespace viekf
