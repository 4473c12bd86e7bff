// viekf_resident_prop.hpp -- resident family: the propagate (dynamics hand-over, low-rank coupling set-up, body strips).
#pragma once
#include "viekf_resident_common.hpp"

namespace viekf {


// Rarely-executed, register-hungry pieces are kept out of line so that they do not inflate the
// register allocation of the sweep loops that hold P.
__device__ RES_INLINE void res_body_phase(const double* xs, const double* u, const DevParams* p, BodyCtx* ctx,
                                            double* xdb, double* Abb, double* Gb) {
  double ub[6];
  q_rota(p->q_b_u, u, ub);
  q_rota(p->q_b_u, u + 3, ub + 3);
  // (the context is built in registers and handed to LDS once: worked on in place, every store to A / G -- which may alias
  //  it as far as the compiler knows -- forces the fields to be re-read from LDS, 10 k clk of single-lane latency)
  BodyCtx c;
  body_ctx(xs, ub, *p, c);
  body_dynamics<false>(c, *p, xdb, Abb, Gb);   // the service wave cleared xdb / Abb / Gb cooperatively
  *ctx = c;
}

// one feature's share of the propagate set-up on the SERVICE wave: dynamics, Phi_ff, state step.  The Jacobian blocks are
// handed to the worker waves RAW, in the EVEN slots of the feature's own three Z rows (row r, slot 2c: c = 0..2 Afv[r][c],
// 3..5 Afg[r][c-3], 6..8 Aff[r][c-6]); a worker thread per row expands them into D and Gs (res_feature_expand_row: odd slots
// and 18..23, so nothing it reads is overwritten), off this wave's serial path.  The even slots receive Ut afterwards.
__device__ RES_INLINE void res_feature_phase(int f, int len, double dt, double* xs, const BodyCtx* ctx, double* Z,
                                             double* phiff) {
  double* z0 = Z + (3 * f) * ZS;
  if (f < len) {
    double xd3[3], Afv[9], Afg[9], Aff[9];
    const double qz[4] = {xs[xZ + 5 * f], xs[xZ + 5 * f + 1], xs[xZ + 5 * f + 2], xs[xZ + 5 * f + 3]};
    const double rho = xs[xZ + 5 * f + 4];
    const BodyCtx c = *ctx;   // (a register copy: the stores below may alias the LDS one as far as the compiler knows)
    feature_dynamics(qz, rho, c, xd3, Afv, Afg, Aff);
    double Aff2[9];
    mm<3, 3, 3>(Aff, Aff, Aff2);
#pragma unroll
    for (int e = 0; e < 9; e++) {
      const double id = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
      phiff[9 * f + e] = id + Aff[e] * dt + Aff2[e] * (0.5 * dt * dt);
    }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c3 = 0; c3 < 3; c3++) {
        z0[r * ZS + 2 * c3] = Afv[r * 3 + c3]; z0[r * ZS + 2 * (3 + c3)] = Afg[r * 3 + c3]; z0[r * ZS + 2 * (6 + c3)] = Aff[r * 3 + c3];
      }
    double qn[4];
    q_feat_boxplus_fast(qz, xd3[0] * dt, xd3[1] * dt, qn);
    double* xf = xs + xZ + 5 * f;
    xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
    xf[4] = rho + xd3[2] * dt;
  } else {  // inactive slot: Phi = I, G = 0
    for (int r = 0; r < 3; r++)
      for (int e = 0; e < 9; e++) z0[r * ZS + 2 * e] = 0.0;
    for (int e = 0; e < 9; e++) phiff[9 * f + e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
  }
}

// Worker side of the hand-over, one thread per row r of feature f: the raw blocks (see above) -> row r of
//   D = [M1 | M3 | M2]  in the odd slots 2k+1,  Gs = Gd_f sqrt(Qu)  in slots 18..23, with
//   Gd_f = dt ((dt/2) (Afv + dt/3 Aff Afv) G_b[vel rows] + (dt^2/6) Afv (A_v G_b) + [0 | (I + Aff dt/2 + Aff^2 dt^2/6) Afg])
//   (vi_ekf.cpp:302 restricted to the feature rows; G_b has no bias rows, vi_ekf_dyn.cpp:74-79)
// (row-wise, operands re-read from LDS: the whole-feature form held ~100 doubles live next to the thread's blocks of P)
__device__ RES_INLINE void res_feature_expand_row(int f, int r, double dt, double* Z, const double* Gb, const double* AvG,
                                                  const double* sqrtQu) {
  const double* z0 = Z + (3 * f) * ZS;
  double* zr = Z + (3 * f + r) * ZS;
  auto raw = [&](int row, int c) { return z0[row * ZS + 2 * c]; };   // c: 0..2 Afv, 3..5 Afg, 6..8 Aff
  const double a0 = raw(r, 6), a1 = raw(r, 7), a2 = raw(r, 8);       // Aff[r][:]
  double AAv[3], AAg[3], A2r[3], afv[3], afg[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    afv[j] = raw(r, j); afg[j] = raw(r, 3 + j);
    AAv[j] = a0 * raw(0, j) + a1 * raw(1, j) + a2 * raw(2, j);
    AAg[j] = a0 * raw(0, 3 + j) + a1 * raw(1, 3 + j) + a2 * raw(2, 3 + j);
    A2r[j] = a0 * raw(0, 6 + j) + a1 * raw(1, 6 + j) + a2 * raw(2, 6 + j);
  }
  const double ar[3] = {a0, a1, a2};
  double mff[3];
#pragma unroll
  for (int j = 0; j < 3; j++) mff[j] = ((j == r) ? 1.0 : 0.0) + ar[j] * (0.5 * dt) + A2r[j] * (dt * dt * (1.0 / 6.0));
#pragma unroll
  for (int k = 0; k < 6; k++) {
    double a = 0.0, b = 0.0;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      a += (afv[j] + (dt * (1.0 / 3.0)) * AAv[j]) * Gb[(dxVEL + j) * 6 + k];
      b += afv[j] * AvG[j * 6 + k];
    }
    double g = a * (0.5 * dt) + b * (dt * dt * (1.0 / 6.0));
    if (k >= 3) g += mff[0] * raw(0, k) + mff[1] * raw(1, k) + mff[2] * raw(2, k);   // (Mff Afg)[r][k-3]
    zr[18 + k] = g * dt * sqrtQu[k];
  }
#pragma unroll
  for (int j = 0; j < 3; j++) {
    zr[2 * j + 1] = (afv[j] + (0.5 * dt) * AAv[j]) * dt;          // M1
    zr[2 * (3 + j) + 1] = afv[j] * (0.5 * dt * dt);               // M3
    zr[2 * (6 + j) + 1] = (afg[j] + (0.5 * dt) * AAg[j]) * dt;    // M2
  }
}

// fix_depth of one feature after the propagate (vi_ekf_helper.cpp:128-156, called at vi_ekf.cpp:311): the state here, the
// covariance edit through the fix mailbox (applied by the worker that owns the feature's diagonal block)
__device__ RES_INLINE void res_fix_depth(double* xf, const DevParams* p, double* fixadd_slot, double* fixset_slot,
                                         double* fixany, unsigned* flag) {
  double rho = xf[4];
  fix_depth_rule(rho, 1.0 / (2.0 * p->min_depth), *flag, [&](double e2) { *fixadd_slot = e2; *fixany = 1.0; },
                 [&] { *fixset_slot = 1.0; *fixany = 1.0; });
  xf[4] = rho;
}


// The six BODY-ONLY quantities of the set-up -- Phi_bb / M_bb, Psi P_bb, T16, Gs_b, Pi, Xi: they involve the 16 x 16 body blocks
// alone, no feature row and no register block -- on the PRIMARY service wave (res_service_setup: the single-propagate kernels
// that run the set-up under the load of P), which would otherwise only wait between B1p and B3p.
// Every element is the expression the worker waves evaluate in the old order (res_prop_setup below), on the same operands, its sum
// running k = 0 .. 15 in the same order; which lane evaluates an element, and what it evaluates next to it, does not enter its
// value, so the two orders agree bit for bit (tests/test_gpu_service_setup.py).  What differs is how the sums are laid out in
// time.  One wave has a third of the workers' lanes and so two to four elements of each quantity per lane: run one after the other,
// each a chain of 16 dependent multiply-adds behind four exposed LDS round trips, the chain took longer than everything the workers
// do meanwhile and the step got SLOWER (profiles/service_setup/README.md).  So the sums of ALL elements of a stage run side by
// side (res_dots: one accumulator per element, k outermost): seven or eight independent chains share each round trip.  A lane whose
// element takes no sum (the E_v / E_g rows of Psi) or does not exist runs its sum on clamped operands and drops the result.
// The worker-side loops do NOT share this text: with calls to common per-element functions in place every kernel of the family,
// the multi-propagate ones included, compiled to a different instruction stream (branch polarities of the three conditional
// sums, index arithmetic of the <7,3> set-up), so the old statements stay where they stood -- a change to one of the six has to be
// made in both places.
template <int NE>
__device__ __forceinline__ void res_dots(const double* const (&x)[NE], const double* const (&y)[NE], const int (&ys)[NE],
                                         double (&acc)[NE]) {
#pragma unroll
  for (int j = 0; j < NE; j++) acc[j] = 0.0;
#pragma unroll 4
  for (int k = 0; k < 16; k++)
#pragma unroll
    for (int j = 0; j < NE; j++) acc[j] += x[j][k] * y[j][k * ys[j]];   // element j: sum_k x[k] y[k ys]
}
__device__ __forceinline__ int res_clamp3(int v) { return min(max(v, 0), 2); }
// Stages (a) Phi_bb, M_bb, Phi_bb^T, Psi P_bb and (b) T16, Gs_b, Pi, ordered by wave_lds_sync (one wave: no barrier).  Everything
// they read is in LDS by B1p (A_bb, G_b: this wave's dynamics; P_bb: loaded ahead of B0; sqrt(Qu): the prologue) and nothing they
// write is touched by the workers' share of the interval (the expansion of the feature rows and V).  Pi must be complete at B2p,
// ahead of the workers' Ut product.  LDSC: sqrt(Qu) from the LDS copy (see res_prop_setup).
template <bool LDSC>
__device__ __forceinline__ void res_prop_setup_body_service(const StreamArgs& a, const ResShared& S, int lane, double dt) {
  const DevParams& prm = a.prm(uniform_filter(S.b));
  {   // (a)  items 0..3: Phi_bb / M_bb element lane + 64 j;  4..6: Psi P_bb element lane + 64 (j - 4) < 144
    const double* x[7]; const double* y[7];
    const int ys[7] = {16, 16, 16, 16, 16, 16, 16};
    double acc[7];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int e = lane + 64 * j; x[j] = S.Abb + (e >> 4) * 16; y[j] = S.Abb + (e & 15); }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const int e = lane + 64 * j, q = e >> 4;
      x[4 + j] = S.Abb + (dxVEL + res_clamp3(q - 3)) * 16; y[4 + j] = S.Pbb + (e & 15);
    }
    res_dots<7>(x, y, ys, acc);
#pragma unroll
    for (int j = 0; j < 4; j++) {   // body transition blocks (vi_ekf.cpp:302-303)
      const int e = lane + 64 * j, r = e >> 4, c = e & 15;
      const double a2 = acc[j];
      const double id = (r == c) ? 1.0 : 0.0, av = S.Abb[e];
      S.Mbb[e] = id + av * (0.5 * dt) + a2 * (dt * dt * (1.0 / 6.0));
      const double ph = id + av * dt + a2 * (0.5 * dt * dt);
      S.Phibb[e] = ph;
      S.PhibbT[c * 16 + r] = ph;
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {   // Psi P_bb: rows E_v, A_bb[vel rows], E_g of P_bb
      const int e = lane + 64 * j, q = e >> 4, c = e & 15;
      if (e < ZK * 16) {
        double v;
        if (q < 3) v = S.Pbb[(dxVEL + q) * 16 + c];
        else if (q >= 6) v = S.Pbb[(dxB_G + q - 6) * 16 + c];
        else v = acc[4 + j];
        S.PsiP[e] = v;
      }
    }
  }
  wave_lds_sync();
  {   // (b)  items 0..3: T16 element lane + 64 j;  4..5: Gs_b element lane + 64 (j - 4) < 96;  6..7: Pi element lane + 64 (j - 6) < 81
    const double* x[8]; const double* y[8];
    const int ys[8] = {16, 16, 16, 16, 6, 6, 1, 1};
    double acc[8];
#pragma unroll
    for (int j = 0; j < 4; j++) { const int e = lane + 64 * j; x[j] = S.Phibb + (e >> 4) * 16; y[j] = S.Pbb + (e & 15); }
#pragma unroll
    for (int j = 0; j < 2; j++) { const int e = min(lane + 64 * j, 95); x[4 + j] = S.Mbb + (e / 6) * 16; y[4 + j] = S.Gb + e % 6; }
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const int e = min(lane + 64 * j, ZK * ZK - 1), q = e / ZK, jj = e - q * ZK;
      x[6 + j] = S.PsiP + q * 16; y[6 + j] = S.Abb + (dxVEL + res_clamp3(jj - 3)) * 16;
    }
    res_dots<8>(x, y, ys, acc);
#pragma unroll
    for (int j = 0; j < 4; j++) S.T16[lane + 64 * j] = acc[j];
#pragma unroll
    for (int j = 0; j < 2; j++) {   // Gs_b = M_bb G_b dt sqrt(Qu)
      const int e = lane + 64 * j, k = e % 6;
      if (e < 96) S.Gdb[e] = acc[4 + j] * dt * (LDSC ? S.sm[res_sm::SQRTQU + k] : prm.sqrtQu[k]);
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {   // Pi = (Psi P_bb) Psi^T
      const int e = lane + 64 * j, q = e / ZK, jj = e - q * ZK;
      if (e < ZK * ZK) {
        const double* pr = S.PsiP + q * 16;
        double v;
        if (jj < 3) v = pr[dxVEL + jj];
        else if (jj >= 6) v = pr[dxB_G + jj - 6];
        else v = acc[6 + j];
        S.Pi[e] = v;
      }
    }
  }
}
// Stage (c), Xi = Psi T16^T (T16^T = P_bb Phi_bb^T): nothing the workers read; T16, Xi, Gs_b and Phi_bb^T are read next by
// res_prop_body, on this same wave, behind B3p.  Runs behind B2p (the workers' Ut product needs no part of it).
__device__ __forceinline__ void res_prop_setup_xi_service(const ResShared& S, int lane) {
  const double* x[3]; const double* y[3];
  const int ys[3] = {1, 1, 1};
  double acc[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int e = lane + 64 * j, q = e >> 4;
    x[j] = S.Abb + (dxVEL + res_clamp3(q - 3)) * 16; y[j] = S.T16 + (e & 15) * 16;
  }
  res_dots<3>(x, y, ys, acc);
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int e = lane + 64 * j, q = e >> 4, c = e & 15;
    if (e < ZK * 16) {
      double v;
      if (q < 3) v = S.T16[c * 16 + dxVEL + q];
      else if (q >= 6) v = S.T16[c * 16 + dxB_G + q - 6];
      else v = acc[j];
      S.Xi[e] = v;
    }
  }
}

// Propagate set-up on the worker waves (LDS only; see the header of this file for the algebra).  Three intervals:
//   [B1p..B2p]  Phi_bb / M_bb, the per-feature expansion raw blocks -> D, Gs, V = Phi_ff P[feat, body] (in place), Psi P_bb
//   [B2p..B2q]  Gs_b = M_bb G_b dt sqrt(Qu), T16 = Phi_bb P_bb, Pi = Psi P_bb Psi^T
//   [B2q..B3p]  Ut = D Pi / 2 + V Psi^T  (the even Z slots), Xi = Psi T16^T
// Barriers B1p, B2p, B2q inside; the caller continues with B3p.
// LDSC: sqrt(Qu) from the resident family's LDS copy (res_sm::SQRTQU, viekf_fused_lds.hpp) -- read from memory, the constant's round
// trip sits inside an interval the whole workgroup waits on, once per interval.  (The tile family's sm has no such words.)
// hook(k), k = 0 .. 2 as std::integral_constant: called behind B1p, B2p and B2q (the worker's spread block loads)
// SS (res_service_setup): the six body-only loops are the service wave's (res_prop_setup_body_service, _xi_service); two intervals are left,
//   [B1p..B2p]  the per-feature expansion and V          [B2p..B3p]  Ut
// B2q is gone on both sides; hook(0) is called behind B1p, hook(1) behind B2p and hook(2) where VIEKF_SERVICE_SETUP_CHUNKS says.
struct ResNoHook { template <class K> __device__ __forceinline__ void operator()(K) const {} };
template <int TW, bool LDSC = false, class Hook = ResNoHook, bool SS = false>
__device__ __forceinline__ void res_prop_setup(const StreamArgs& a, const ResShared& S, int tid, const Hook& hook = Hook()) {
  const int nf = S.nf, N = S.N;
  const DevParams& prm = a.prm(uniform_filter(S.b));
  double* Pbc = S.Pbc; double* Pbb = S.Pbb;
  double* Z = S.Z; double* phiff = S.phiff;
  double* Phibb = S.Phibb; double* Mbb = S.Mbb; double* Gdb = S.Gdb; double* T16 = S.T16;
  __syncthreads();  // B1p : body Jacobian, raw feature blocks and Phi_ff ready (service), and this propagate's dt
  const double dt = S.sm[res_sm::DT];   // (the same word in both families: tile_sm::DT)
  hook(std::integral_constant<int, 0>{});

  // ---- [B1p..B2p]
  for (int e = tid; e < nf; e += TW) res_feature_expand_row(e / 3, e % 3, dt, Z, S.Gb, S.AvG, LDSC ? S.sm + res_sm::SQRTQU : prm.sqrtQu);
  if (!SS) {   // (SS: the service wave's, see res_prop_setup_body_service)
    for (int e = TW - 1 - tid; e < 256; e += TW) {   // body transition blocks (vi_ekf.cpp:302-303), from the last threads
      const int r = e >> 4, c = e & 15;
      double a2 = 0.0;
#pragma unroll 4
      for (int k = 0; k < 16; k++) a2 += S.Abb[r * 16 + k] * S.Abb[k * 16 + c];
      const double id = (r == c) ? 1.0 : 0.0, av = S.Abb[e];
      Mbb[e] = id + av * (0.5 * dt) + a2 * (dt * dt * (1.0 / 6.0));
      const double ph = id + av * dt + a2 * (0.5 * dt * dt);
      Phibb[e] = ph;
      S.PhibbT[c * 16 + r] = ph;   // transposed copy: lanes that differ in the OUTPUT column read consecutive words
    }
    for (int e = TW - 1 - tid; e < ZK * 16; e += TW) {   // Psi P_bb: rows E_v, A_bb[vel rows], E_g of P_bb
      const int q = e >> 4, c = e & 15;
      double v;
      if (q < 3) v = Pbb[(dxVEL + q) * 16 + c];
      else if (q >= 6) v = Pbb[(dxB_G + q - 6) * 16 + c];
      else {
        v = 0.0;
#pragma unroll 4
        for (int k = 0; k < 16; k++) v += S.Abb[(dxVEL + q - 3) * 16 + k] * Pbb[k * 16 + c];
      }
      S.PsiP[e] = v;
    }
  }
  for (int e = tid; e < 16 * N; e += TW) {   // V = Phi_ff[f] P[f, body], in place: item = (feature f, body column k)
    const int f = e >> 4, k = e & 15;
    const double* ff = phiff + 9 * f;
    double* pc = Pbc + (3 * f) * 16 + k;
    const double p0 = pc[0], p1 = pc[16], p2 = pc[32];
    pc[0] = ff[0] * p0 + ff[1] * p1 + ff[2] * p2;
    pc[16] = ff[3] * p0 + ff[4] * p1 + ff[5] * p2;
    pc[32] = ff[6] * p0 + ff[7] * p1 + ff[8] * p2;
  }
  RES_STAMP(S, tid == 0, 77);
  __syncthreads();  // B2p
  RES_STAMP(S, tid == 0, 78);
  hook(std::integral_constant<int, 1>{});

  // ---- [B2p..B2q]
  if (!SS) {
    for (int e = tid; e < 256; e += TW) {
      const int r = e >> 4, c = e & 15;
      double sv = 0.0;
#pragma unroll 4
      for (int k = 0; k < 16; k++) sv += Phibb[r * 16 + k] * Pbb[k * 16 + c];
      T16[e] = sv;
    }
    for (int e = TW - 1 - tid; e < 96; e += TW) {
      const int r = e / 6, k = e % 6;
      double sv = 0.0;
#pragma unroll 4
      for (int c = 0; c < 16; c++) sv += Mbb[r * 16 + c] * S.Gb[c * 6 + k];
      Gdb[e] = sv * dt * (LDSC ? S.sm[res_sm::SQRTQU + k] : prm.sqrtQu[k]);
    }
    for (int e = tid; e < ZK * ZK; e += TW) {   // Pi = (Psi P_bb) Psi^T
      const int q = e / ZK, j = e - q * ZK;
      const double* pr = S.PsiP + q * 16;
      double v;
      if (j < 3) v = pr[dxVEL + j];
      else if (j >= 6) v = pr[dxB_G + j - 6];
      else {
        v = 0.0;
#pragma unroll 4
        for (int k = 0; k < 16; k++) v += pr[k] * S.Abb[(dxVEL + j - 3) * 16 + k];
      }
      S.Pi[e] = v;
    }
    __syncthreads();  // B2q
  }
  if (!SS || VIEKF_SERVICE_SETUP_CHUNKS == 0) hook(std::integral_constant<int, 2>{});

  // ---- [B2q..B3p]
  // Ut = [D | V] [Pi / 2 ; Psi^T]  (nf x 25)(25 x 9) on the matrix cores, one 16-row tile per wave and turn, 7 k-steps (as
  // 1350 dot products this interval was LDS-bound: 50 operand reads per output).  A result lane holds column lr = lane & 15
  // of rows lk + 4 r (lk = lane >> 4) of the tile; columns 9..15 of the right-hand side are zero.
  {
    const int lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
    double bv[7];
    int aoff[7];     // where k = 4 sk + lk sits: D[k] in the Z row (odd slots), V[k - 9] in the Pbc row, k >= 25: nowhere
#pragma unroll
    for (int sk = 0; sk < 7; sk++) {
      const int k = 4 * sk + lk, c = k - ZK;
      double v = 0.0;
      if (lr < ZK) {
        if (k < ZK) v = 0.5 * S.Pi[k * ZK + lr];
        else if (c < 16) v = (lr < 3) ? ((c == dxVEL + lr) ? 1.0 : 0.0)
                           : ((lr >= 6) ? ((c == dxB_G + lr - 6) ? 1.0 : 0.0) : S.Abb[(dxVEL + lr - 3) * 16 + c]);
      }
      bv[sk] = v;
      aoff[sk] = (k < ZK) ? (2 * k + 1) : ((c < 16) ? (0x100 | c) : -1);
    }
    for (int t = wv; t * 16 < nf; t += TW / 64) {
      const int ar = min(16 * t + lr, nf - 1);
      v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int sk = 0; sk < 7; sk++) {
        const int o = aoff[sk];
        const double av = (o < 0) ? 0.0 : ((o & 0x100) ? Pbc[ar * 16 + (o & 0xff)] : Z[ar * ZS + o]);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[sk], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r4 = 0; r4 < 4; r4++) {
        const int row = 16 * t + lk + 4 * r4;
        if (row < nf && lr < ZK) Z[row * ZS + 2 * lr] = acc[r4];
      }
      if (SS && VIEKF_SERVICE_SETUP_CHUNKS == 1 && t == wv) hook(std::integral_constant<int, 2>{});   // behind the first turn
    }
    if (SS && VIEKF_SERVICE_SETUP_CHUNKS == 1 && wv * 16 >= nf) hook(std::integral_constant<int, 2>{});   // (a wave without a turn)
  }
  if (!SS) {
    for (int e = TW - 1 - tid; e < ZK * 16; e += TW) {   // Xi = Psi T16^T  (T16^T = P_bb Phi_bb^T)
      const int q = e >> 4, c = e & 15;
      double v;
      if (q < 3) v = T16[c * 16 + dxVEL + q];
      else if (q >= 6) v = T16[c * 16 + dxB_G + q - 6];
      else {
        v = 0.0;
#pragma unroll 4
        for (int k = 0; k < 16; k++) v += S.Abb[(dxVEL + q - 3) * 16 + k] * T16[c * 16 + k];
      }
      S.Xi[e] = v;
    }
  }
}

// P+[feature rows, body columns] = V Phi_bb^T + D Xi + Gs Gs_b^T, in LDS and in place (a tile's rows are read before they are
// written, by the same wave), and the body block (-> Mbb).  (nf x 16)(16 x 16) + (nf x 16)(16 x 16) on the matrix cores, one
// 16-row tile per wave and turn, 4 + 4 k-steps: the second product's k runs over D[0..8], Gs[0..5] and one zero.
// LDSC: Qx of the 16 body rows from the resident family's LDS copy (res_sm::QXB: see res_prop_setup), else StreamArgs::qx.
template <int TW, bool LDSC = false>
__device__ __forceinline__ void res_prop_body(const StreamArgs& a, const ResShared& S, int tid) {
  const int nf = S.nf;
  double* Pbc = S.Pbc;
  const double* Z = S.Z; double* Gdb = S.Gdb; double* T16 = S.T16;
  {
    const int lane = tid & 63, wv = tid >> 6, lr = lane & 15, lk = lane >> 4;
    constexpr int step = TW / 64;
    // the right-hand operands do not depend on the tile: loaded once; two tiles per turn, so that one tile's dependent
    // MFMA chain runs in the shadow of the other's
    double bph[4], bdx[4];
    int zoff[4];   // slot of k = 4 sk + lk in a Z row: D[k] at 2k+1, Gs[k-9] at 18 + k - 9, k = 15: none
#pragma unroll
    for (int sk = 0; sk < 4; sk++) {
      const int k = 4 * sk + lk;
      bph[sk] = S.PhibbT[k * 16 + lr];
      bdx[sk] = (k < ZK) ? S.Xi[k * 16 + lr] : ((k < ZK + 6) ? Gdb[lr * 6 + (k - ZK)] : 0.0);
      zoff[sk] = (k < ZK) ? (2 * k + 1) : ((k < ZK + 6) ? (18 + k - ZK) : -1);
    }
    for (int t = wv; t * 16 < nf; t += 2 * step) {
      const int t1 = t + step;
      const int r0 = min(16 * t + lr, nf - 1), r1 = min(16 * t1 + lr, nf - 1);
      double a0[8], a1[8];
#pragma unroll
      for (int sk = 0; sk < 4; sk++) {
        a0[sk] = Pbc[r0 * 16 + 4 * sk + lk]; a1[sk] = Pbc[r1 * 16 + 4 * sk + lk];
        a0[4 + sk] = (zoff[sk] >= 0) ? Z[r0 * ZS + zoff[sk]] : 0.0;
        a1[4 + sk] = (zoff[sk] >= 0) ? Z[r1 * ZS + zoff[sk]] : 0.0;
      }
      v4f64 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int sk = 0; sk < 8; sk++) {
        const double bv = sk < 4 ? bph[sk] : bdx[sk - 4];
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[sk], bv, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[sk], bv, acc1, 0, 0, 0);
      }
      // (every lane of the wave has its operands before any lane stores: the stores depend on the MFMA results)
#pragma unroll
      for (int r4 = 0; r4 < 4; r4++) {
        const int row0 = 16 * t + lk + 4 * r4, row1 = 16 * t1 + lk + 4 * r4;
        if (row0 < nf) Pbc[row0 * 16 + lr] = acc0[r4];
        if (row1 < nf) Pbc[row1 * 16 + lr] = acc1[r4];
      }
    }
  }
  // body block  P_bb+ = T16 Phi_bb^T + Gs_b Gs_b^T + Qx : one 16 x 16 tile, 4 + 2 k-steps, on the first wave
  if (tid < 64) {
    const int lr = tid & 15, lk = tid >> 4;
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int sk = 0; sk < 4; sk++) {
      const int k = 4 * sk + lk;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(T16[lr * 16 + k], S.PhibbT[k * 16 + lr], acc, 0, 0, 0);   // rows r = lr | cols c = lr
    }
#pragma unroll
    for (int sk = 0; sk < 2; sk++) {
      const int k = 4 * sk + lk;                                   // 0..7, the input-noise columns are k < 6
      const double gv = (k < 6) ? Gdb[lr * 6 + k] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(gv, gv, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r4 = 0; r4 < 4; r4++) {
      const int r = lk + 4 * r4, c = lr;                           // a result lane holds column lr of rows lk + 4 r4
      S.Mbb[r * 16 + c] = acc[r4] + ((r == c) ? (LDSC ? S.sm[res_sm::QXB + r] : a.qx(uniform_filter(S.b))[r]) : 0.0); // P_bb+ staged in Mbb (T16 / Pbb are still being read)
    }
  }
}

}  // namespace viekf
