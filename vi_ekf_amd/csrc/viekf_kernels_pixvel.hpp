// viekf_kernels_pixvel.hpp -- the PIXEL_VEL measurement (viekf_pixvel_model.hpp): the update kernel, one entry per launch, the
// read-only evaluation, the flow of a frame's features by id and the id -> slot lookup of the intake's pixel-velocity step.
// Defines kernels: included from viekf_dispatch.hpp only.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"
#include "viekf_pixvel_lds.hpp"
#include "viekf_pixvel_model.hpp"

namespace viekf {

// The arithmetic both routes share, stated once so that they contract alike: route 1 must give route 0's bits.
//   L(i, j) of the partial update;  a gain element K[i][q] = sum_p W[i][p] S^-1[p][q];  one element of the correction;
//   one applied entry's downdate of one element, v -= L (K[hi] . W[lo]) with hi = max(i, j), lo = min(i, j).
__device__ __forceinline__ double pixvel_L(bool partial, double li, double lj) { return partial ? (lj + li - li * lj) : 1.0; }
__device__ __forceinline__ double pixvel_gain(double w0, double w1, const double* Si, int q) {
  double k = 0.0;
  k += w0 * Si[q];
  k += w1 * Si[2 + q];
  return k;
}
__device__ __forceinline__ double pixvel_dx(double l, double k0, double k1, double r0, double r1) {
  double s = 0.0;
  s += (l * k0) * r0;
  s += (l * k1) * r1;
  return s;
}
__device__ __forceinline__ double pixvel_downdate(double v, double L, double k0, double k1, double w0, double w1) {
  double t = 0.0;
  t += k0 * w0;
  t += k1 * w1;
  return v - L * t;
}
// one row of W = P H^T: the nine elements of the row of P that H's columns name (col(c)), times Hc (sm[0 .. 17])
template <class Col>
__device__ __forceinline__ void pixvel_w(const double* sm, Col&& col, double& w0, double& w1) {
  w0 = 0.0;
  w1 = 0.0;
#pragma unroll
  for (int c = 0; c < kPixvelCols; c++) {
    const double pv = col(c);
    w0 += pv * sm[c];
    w1 += pv * sm[kPixvelCols + c];
  }
}
// S (row-major 2 x 2) = H W[cols] + R + gyro_var J J^T from the model's Hc (sm[0 .. 17]) and the rows of W that H's columns
// name (wrow(c, q) = W[cols[c]][q]); then S^-1, the gate's verdict and S^-1 into sm[20 .. 24].  One lane.
template <class WRow>
__device__ __forceinline__ void pixvel_gate(double* sm, const double* R, double gyro_var, WRow&& wrow) {
  double S[4], Si[4];
  for (int p = 0; p < 2; p++)
    for (int q = 0; q < 2; q++) {
      double s = 0.0, jj = 0.0;
      for (int c = 0; c < kPixvelCols; c++) s += sm[p * kPixvelCols + c] * wrow(c, q);
      for (int k = 3; k < 6; k++) jj += sm[p * kPixvelCols + k] * sm[q * kPixvelCols + k];
      S[p * 2 + q] = s + (R[p + q * 2] + gyro_var * jj);
    }
  small_inverse_dev(2, S, Si);
  double mahal = 0.0;
  for (int q = 0; q < 2; q++) { double t = 0.0; for (int p = 0; p < 2; p++) t += sm[18 + p] * Si[p * 2 + q]; mahal += t * sm[18 + q]; }
  for (int i = 0; i < 4; i++) sm[20 + i] = Si[i];
  sm[24] = (mahal > kGateMahal) ? 1.0 : 0.0;   // :234-239
}

// ------------------------------------------------------------------------------------------------
// One PIXEL_VEL measurement per filter: entry m of the call's [B][M] rows.  VIEKF::update (vi_ekf_meas.cpp:196-278) with the
// structure of k_update_generic -- nine non-zero columns of H instead of at most six, rank 2, and the gyro sample's own noise
// in the effective R:  S = H P H^T + R + gyro_var J J^T, J the B_G block of H (d zhat / d omega = -d zhat / d b_g).
// The sweep  P_ij -= Lambda_ij (K_hi . W_lo)  is the Joseph form with that R at the optimal gain (K S = W).
// One workgroup per filter, P in memory and read whole (the columns of W): the caller brings P to the full form.
// The rules of an entry and their order: include/viekf_pixvel.h.
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_update_pixvel(StreamArgs a, int M, int m,
                                                     const int* __restrict__ slot_all,      // [B][M]
                                                     const double* __restrict__ z_all,      // [B][M][2]
                                                     const double* __restrict__ gyro_all,   // [B][3]
                                                     const double* __restrict__ R_all, long r_stride_b, long r_stride_m,
                                                     double gyro_var,
                                                     const unsigned char* __restrict__ active_all,   // [B][M] or NULL
                                                     int* __restrict__ result_all) {                 // [B][M] or NULL
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n, ld = a.ld;
  const DevParams& prm = *a.dp;
  const PixvelLds lds(a.nxs, n);
  double* xs = smem + lds.xs;
  double* W = smem + lds.W;
  double* K = smem + lds.K;
  double* lam = smem + lds.lam;
  double* sm = smem + lds.sm;
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const long at = (long)b * M + m;
  const int act = active_all ? active_all[at] : 1;
  int* res_out = (result_all && tid == 0) ? &result_all[at] : nullptr;
  if (act == 2) { if (res_out) *res_out = -1; return; }   // this filter skips the entry
  const int slot = slot_all[at];
  if (slot < 0 || slot >= len) { if (res_out) *res_out = (slot < 0) ? -1 : 3; return; }
  const double* z = z_all + 2 * at;
  const double* gyro = gyro_all + 3L * b;
  if (z[0] != z[0] || z[1] != z[1] || gyro[0] != gyro[0] || gyro[1] != gyro[1] || gyro[2] != gyro[2]) {
    if (res_out) *res_out = 2;   // MEAS_NAN
    return;
  }
  unsigned flag = 0;
  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lambda[i];
  __syncthreads();
  if (act == 0) {   // :230 -- an inactive measurement only runs fix_depth
    for (int f = tid; f < len; f += T) fix_depth_one(xs, P, ld, f, prm, flag);
    __syncthreads();
    for (int i = tid; i < xZ + 5 * len; i += T) xg[i] = xs[i];
    if (res_out) *res_out = 0;
    if (flag) atomicOr(&a.flags[b], flag);
    return;
  }
  if (tid == 0) {   // the model: zhat, the nine columns of H, the residual
    double zhat[2], Hc[2 * kPixvelCols];
    pixel_vel_model(xs, slot, gyro, prm, zhat, Hc);
    for (int i = 0; i < 2 * kPixvelCols; i++) sm[i] = Hc[i];
    sm[18] = z[0] - zhat[0];
    sm[19] = z[1] - zhat[1];
  }
  __syncthreads();
  int cols[kPixvelCols];
  pixel_vel_cols(slot, cols);
  // W = P H^T (n x 2): a combination of the nine columns
  for (int i = tid; i < nact; i += T) {
    double w0, w1;
    pixvel_w(sm, [&](int c) { return P[i + (long)cols[c] * ld]; }, w0, w1);
    W[2 * i] = w0;
    W[2 * i + 1] = w1;
  }
  __syncthreads();
  if (tid == 0) {   // S = H W[cols] + R + gyro_var J J^T, inverse, gate
    const double* R = R_all + b * r_stride_b + m * r_stride_m;   // column-major 2 x 2
    pixvel_gate(sm, R, gyro_var, [&](int c, int q) { return W[2 * cols[c] + q]; });
  }
  __syncthreads();
  if (sm[24] != 0.0) { if (res_out) *res_out = 1; return; }   // gated: returns before fix_depth
  int bad = 0;
  for (int i = tid; i < nact; i += T)
    for (int q = 0; q < 2; q++) {
      const double k = pixvel_gain(W[2 * i], W[2 * i + 1], sm + 20, q);
      K[2 * i + q] = k;
      if (k != k) bad = 1;
    }
  for (int i = 0; i < 2 * kPixvelCols; i++) if (sm[i] != sm[i]) bad = 1;
  bad = __syncthreads_or(bad);
  if (!bad) {   // :247
    const bool partial = prm.use_partial_update != 0;
    const double r0 = sm[18], r1 = sm[19];
    if (tid == 0) {
      double dxb[16], xo[17];
      for (int i = 0; i < 16; i++) {
        dxb[i] = pixvel_dx(partial ? lam[i] : 1.0, K[2 * i], K[2 * i + 1], r0, r1);
      }
      body_boxplus(xs, dxb, xo);
      for (int i = 0; i < 17; i++) xs[i] = xo[i];
    }
    for (int f = tid; f < len; f += T) {
      const int d = 16 + 3 * f;
      double dv[3];
      for (int e = 0; e < 3; e++) {
        dv[e] = pixvel_dx(partial ? lam[d + e] : 1.0, K[2 * (d + e)], K[2 * (d + e) + 1], r0, r1);
      }
      double* xf = xs + xZ + 5 * f;
      double qn[4];
      q_feat_boxplus(xf, dv[0], dv[1], qn);
      xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
      xf[4] += dv[2];
    }
    // a wave walks a column (64 consecutive rows per step), the waves take the columns in turn
    for (int j = tid >> 6; j < nact; j += T / 64) {
      const double lj = lam[j];
      for (int i = tid & 63; i < nact; i += 64) {
        const int hi = max(i, j), lo = min(i, j);   // (exactly symmetric result, as k_update_generic)
        const long at = i + (long)j * ld;
        P[at] = pixvel_downdate(P[at], pixvel_L(partial, lam[i], lj), K[2 * hi], K[2 * hi + 1], W[2 * lo], W[2 * lo + 1]);
      }
    }
  }
  __syncthreads();
  for (int f = tid; f < len; f += T) fix_depth_one(xs, P, ld, f, prm, flag);
  __syncthreads();
  for (int i = tid; i < xZ + 5 * len; i += T) {
    const double v = xs[i];
    if (v != v) flag |= FLAG_NAN;
    if (v > 1e6) flag |= FLAG_BLOWUP;
    xg[i] = v;
  }
  if (res_out) *res_out = 0;
  if (flag) atomicOr(&a.flags[b], flag);
}

// ------------------------------------------------------------------------------------------------
// The fused route: M PIXEL_VEL measurements per filter, applied in order, with the arithmetic of M launches of k_update_pixvel
// -- element for element, through the shared functions above -- and one read and one write of the lower triangle of P.
//
// What an entry needs of the current P is nine columns.  The six body columns (VEL, B_G) ride along as a panel Pb that every
// applied entry downdates (as section 17 of DESIGN.md keeps its body panel).  The feature's three columns are rebuilt
// left-looking (section 18): the start P's column, from global memory, which nobody writes before the trailing pass, minus the
// downdates of the entries applied so far, which their W and S^-1 in LDS give.  fix_depth edits P(rho, rho), which later
// entries only subtract from: those diagonals ride along in D.  Every other element of the lower triangle gets the applied
// entries' downdates in entry order in the trailing pass: loaded once, stored once.  Nothing above the diagonal, at or past
// row / column nact, or in the pad rows is read or written.
// One workgroup per filter; a.si(b) is followed.  The rules of an entry and their order: include/viekf_pixvel.h.
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_update_pixvels(StreamArgs a, int M, int order,
                                                      const int* __restrict__ slot_all,      // [B][M]
                                                      const double* __restrict__ z_all,      // [B][M][2]
                                                      const double* __restrict__ gyro_all,   // [B][3]
                                                      const double* __restrict__ R_all, long r_stride_b, long r_stride_m,
                                                      double gyro_var,
                                                      const unsigned char* __restrict__ active_all,   // [B][M] or NULL
                                                      int* __restrict__ result_all) {                 // [B][M] or NULL
  static_assert(T % 64 == 0, "whole waves");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n, ld = a.ld;
  const DevParams& prm = *a.dp;
  const PixvelsLds lds(a.nxs, n, (n - 16) / 3, M);
  const int nW = lds.nW;
  double* xs = smem + lds.xs;
  double* lam = smem + lds.lam;
  double* D = smem + lds.D;
  double* Pb = smem + lds.Pb;
  double* Fc = smem + lds.Fc;
  double* sm = smem + lds.sm;
  double* Sinv = smem + lds.Si;
  double* Wall = smem + lds.W;
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const int nxa = xZ + 5 * len;
  const bool partial = prm.use_partial_update != 0;
  const long row = (long)b * M;
  const double* gyro = gyro_all + 3L * b;
  const bool gyro_nan = gyro[0] != gyro[0] || gyro[1] != gyro[1] || gyro[2] != gyro[2];
  auto entry_of = [&](int e) { return order ? M - 1 - e : e; };
  auto p_low = [&](int i, int c) { return (i >= c) ? P[i + (long)c * ld] : P[c + (long)i * ld]; };   // (the lower triangle only)
  const int bcol[6] = {dxVEL, dxVEL + 1, dxVEL + 2, dxB_G, dxB_G + 1, dxB_G + 2};

  for (int i = tid; i < nxa; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lambda[i];
  for (int f = tid; f < len; f += T) { const long dR = dxZ + 3 * f + 2; D[f] = P[dR + dR * ld]; }
  for (int i = tid; i < nact; i += T) {
    double v[6];
#pragma unroll
    for (int j = 0; j < 6; j++) v[j] = p_low(i, bcol[j]);
#pragma unroll
    for (int j = 0; j < 6; j++) Pb[j * nW + i] = v[j];
  }

  auto fix_depth_lds = [&](int f, unsigned& flag) {   // fix_depth_one with P(rho, rho) in D
    const int xR = xZ + 5 * f + 4;
    double rho = xs[xR];
    fix_depth_rule(rho, 1.0 / (2.0 * prm.min_depth), flag, [&](double e2) { D[f] += e2; }, [&] { D[f] = prm.P0_feat[2]; });
    xs[xR] = rho;
  };

  unsigned flag = 0;    // (per thread; ORed into the filter's word at the end)
  int napp = 0;         // entries applied so far: the rows of W / Si the next one writes
  bool dirty = false;   // some entry got as far as touching x or P(rho, rho)
  for (int e = 0; e < M; e++) {
    const int m = entry_of(e);
    const long at = row + m;
    const int act = active_all ? active_all[at] : 1;
    int* res_out = (result_all && tid == 0) ? &result_all[at] : nullptr;
    if (act == 2) { if (res_out) *res_out = -1; continue; }   // this filter skips the entry
    const int slot = slot_all[at];
    if (slot < 0 || slot >= len) { if (res_out) *res_out = (slot < 0) ? -1 : 3; continue; }
    const double z0 = z_all[2 * at], z1 = z_all[2 * at + 1];
    if (z0 != z0 || z1 != z1 || gyro_nan) { if (res_out) *res_out = 2; continue; }   // MEAS_NAN
    __syncthreads();   // what the load or the entry before wrote (xs, D, Pb, W, Si); sm and Fc are free again
    if (act == 0) {    // :230 -- an inactive measurement only runs fix_depth
      for (int f = tid; f < len; f += T) fix_depth_lds(f, flag);
      if (res_out) *res_out = 0;
      dirty = true;
      continue;
    }
    if (tid == 0) {   // the model: zhat, the nine columns of H, the residual
      double zhat[2], Hc[2 * kPixvelCols];
      pixel_vel_model(xs, slot, gyro, prm, zhat, Hc);
      for (int i = 0; i < 2 * kPixvelCols; i++) sm[i] = Hc[i];
      sm[18] = z0 - zhat[0];
      sm[19] = z1 - zhat[1];
    }
    int cols[kPixvelCols];
    pixel_vel_cols(slot, cols);
    // the feature's three columns of the current P, left-looking
    for (int idx = tid; idx < 3 * nact; idx += T) {
      const int q = idx / nact, i = idx - q * nact;
      const int c = cols[6 + q];
      double v = p_low(i, c);
      const int hi = max(i, c), lo = min(i, c);
      const double L = pixvel_L(partial, lam[i], lam[c]);
      for (int k = 0; k < napp; k++) {
        const double* Wk = Wall + (long)k * 2 * nW;
        const double* Sk = Sinv + 4 * k;
        v = pixvel_downdate(v, L, pixvel_gain(Wk[hi], Wk[nW + hi], Sk, 0), pixvel_gain(Wk[hi], Wk[nW + hi], Sk, 1), Wk[lo], Wk[nW + lo]);
      }
      if (q == 2 && i == c) v = D[slot];   // (the rho diagonal is current in D, fix_depth's edits included)
      Fc[q * nW + i] = v;
    }
    __syncthreads();
    double* W0 = Wall + (long)napp * 2 * nW;
    double* W1 = W0 + nW;
    for (int i = tid; i < nact; i += T) {
      double w0, w1;
      pixvel_w(sm, [&](int c) { return c < 6 ? Pb[c * nW + i] : Fc[(c - 6) * nW + i]; }, w0, w1);
      W0[i] = w0;
      W1[i] = w1;
    }
    __syncthreads();
    if (tid == 0) {   // S = H W[cols] + R + gyro_var J J^T, inverse, gate
      const double* R = R_all + b * r_stride_b + m * r_stride_m;   // column-major 2 x 2
      pixvel_gate(sm, R, gyro_var, [&](int c, int q) { return (q ? W1 : W0)[cols[c]]; });
    }
    __syncthreads();
    if (sm[24] != 0.0) { if (res_out) *res_out = 1; continue; }   // gated: no fix_depth, no row taken
    const double Si[4] = {sm[20], sm[21], sm[22], sm[23]};
    int bad = 0;
    for (int i = tid; i < nact; i += T)
      for (int q = 0; q < 2; q++) {
        const double k = pixvel_gain(W0[i], W1[i], Si, q);
        if (k != k) bad = 1;
      }
    for (int i = 0; i < 2 * kPixvelCols; i++) if (sm[i] != sm[i]) bad = 1;
    bad = __syncthreads_or(bad);
    const double r0 = sm[18], r1 = sm[19];
    if (!bad) {   // :247
      if (tid == 0) {
        double dxb[16], xo[17];
        for (int i = 0; i < 16; i++)
          dxb[i] = pixvel_dx(partial ? lam[i] : 1.0, pixvel_gain(W0[i], W1[i], Si, 0), pixvel_gain(W0[i], W1[i], Si, 1), r0, r1);
        body_boxplus(xs, dxb, xo);
        for (int i = 0; i < 17; i++) xs[i] = xo[i];
        for (int i = 0; i < 4; i++) Sinv[4 * napp + i] = Si[i];
      }
      // the body panel takes the entry's downdate
      for (int idx = tid; idx < 6 * nact; idx += T) {
        const int j = idx / nact, i = idx - j * nact;
        const int c = bcol[j];
        const int hi = max(i, c), lo = min(i, c);
        Pb[j * nW + i] = pixvel_downdate(Pb[j * nW + i], pixvel_L(partial, lam[i], lam[c]), pixvel_gain(W0[hi], W1[hi], Si, 0),
                                         pixvel_gain(W0[hi], W1[hi], Si, 1), W0[lo], W1[lo]);
      }
    }
    // a thread's features: correction, P(rho, rho), fix_depth and the scan k_update_pixvel makes when it writes x back
    for (int f = tid; f < len; f += T) {
      double* xf = xs + xZ + 5 * f;
      if (!bad) {
        const int d = 16 + 3 * f;
        double dv[3];
        for (int q = 0; q < 3; q++)
          dv[q] = pixvel_dx(partial ? lam[d + q] : 1.0, pixvel_gain(W0[d + q], W1[d + q], Si, 0), pixvel_gain(W0[d + q], W1[d + q], Si, 1), r0, r1);
        double qn[4];
        q_feat_boxplus(xf, dv[0], dv[1], qn);
        xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
        xf[4] += dv[2];
        const int dr = d + 2;
        D[f] = pixvel_downdate(D[f], pixvel_L(partial, lam[dr], lam[dr]), pixvel_gain(W0[dr], W1[dr], Si, 0),
                               pixvel_gain(W0[dr], W1[dr], Si, 1), W0[dr], W1[dr]);
      }
      fix_depth_lds(f, flag);
      for (int q = 0; q < 5; q++) {
        const double v = xf[q];
        if (v != v) flag |= FLAG_NAN;
        if (v > 1e6) flag |= FLAG_BLOWUP;
      }
    }
    if (tid == 0)
      for (int i = 0; i < xZ; i++) {
        const double v = xs[i];
        if (v != v) flag |= FLAG_NAN;
        if (v > 1e6) flag |= FLAG_BLOWUP;
      }
    if (res_out) *res_out = 0;
    dirty = true;
    napp += bad ? 0 : 1;   // W and Si of this entry stay for the entries after it and for the trailing pass
  }
  if (!dirty) return;   // every entry skipped, invalid, NaN or gated: the filter is left as it is
  __syncthreads();
  for (int i = tid; i < nxa; i += T) xg[i] = xs[i];
  for (int f = tid; f < len; f += T) {   // (fix_depth only: the diagonals it edited and no other)
    const long dR = dxZ + 3 * f + 2;
    if (napp > 0 || __double_as_longlong(P[dR + dR * ld]) != __double_as_longlong(D[f])) P[dR + dR * ld] = D[f];
  }
  if (flag) atomicOr(&a.flags[b], flag);
  if (napp == 0) return;
  // ---- the trailing pass: the lower triangle of the active block, rho diagonals excepted.  A lane keeps ROW i (64 consecutive
  //      rows per wave: a column's segment is 512 contiguous bytes); a wave takes UN adjacent columns at a time, loads before
  //      arithmetic; the entries run innermost, in order, on the values held in registers ----
  constexpr int NWV = T / 64, UN = 8;
  const int wid = tid >> 6, lane = tid & 63;
  for (int r0 = 0; r0 < nact; r0 += 64) {
    const int i = r0 + lane;
    const bool valid = i < nact;
    const int ir = valid ? i : 0;
    const double li = lam[ir];
    const bool isrho = i >= dxZ && (i - dxZ) % 3 == 2;
    const int jend = min(r0 + 63, nact - 1);
    for (int j0 = wid * UN; j0 <= jend; j0 += NWV * UN) {
      double p[UN], L[UN];
      bool ok[UN];
#pragma unroll
      for (int u = 0; u < UN; u++) {
        const int j = j0 + u;
        ok[u] = valid && j <= i && !(i == j && isrho);   // (j <= i < nact)
        p[u] = 0.0;
        if (ok[u]) p[u] = P[i + (long)j * ld];
      }
#pragma unroll
      for (int u = 0; u < UN; u++) L[u] = pixvel_L(partial, li, lam[min(j0 + u, nact - 1)]);
      for (int k = 0; k < napp; k++) {
        const double* Wk = Wall + (long)k * 2 * nW;
        const double* Sk = Sinv + 4 * k;
        const double k0 = pixvel_gain(Wk[ir], Wk[nW + ir], Sk, 0), k1 = pixvel_gain(Wk[ir], Wk[nW + ir], Sk, 1);
#pragma unroll
        for (int u = 0; u < UN; u++) {
          const int jc = min(j0 + u, nact - 1);
          p[u] = pixvel_downdate(p[u], L[u], k0, k1, Wk[jc], Wk[nW + jc]);
        }
      }
#pragma unroll
      for (int u = 0; u < UN; u++)
        if (ok[u]) P[i + (long)(j0 + u) * ld] = p[u];
    }
  }
}

// viekf_batch_eval_pixel_vel: zhat [B][2] and, where H is not NULL, H [B][2][n] dense, at the batch's current state -- the device
// function the update kernel uses.  One lane per filter; a slot outside [0, len): zhat and H are NaN.  Nothing is written to the filter.
__global__ __launch_bounds__(64) void k_eval_pixel_vel(StreamArgs a, const int* __restrict__ slot_all, const double* __restrict__ gyro_all,
                                                       double* __restrict__ zhat_out, double* __restrict__ H_out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n;
  const double* xs = a.x + a.si(b) * a.nxs;
  const int slot = slot_all[b];
  const bool ok = slot >= 0 && slot < a.len[b];
  double zhat[2] = {0.0, 0.0}, Hc[2 * kPixvelCols];
  int cols[kPixvelCols];
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (ok) {
    pixel_vel_model(xs, slot, gyro_all + 3L * b, *a.dp, zhat, Hc);
    pixel_vel_cols(slot, cols);
  }
  zhat_out[2L * b] = ok ? zhat[0] : nan;
  zhat_out[2L * b + 1] = ok ? zhat[1] : nan;
  if (!H_out) return;
  double* H = H_out + 2L * b * n;
  for (int i = 0; i < 2 * n; i++) H[i] = ok ? 0.0 : nan;
  if (ok)
    for (int r = 0; r < 2; r++)
      for (int c = 0; c < kPixvelCols; c++) H[(long)r * n + cols[c]] = Hc[r * kPixvelCols + c];
}

// viekf_pixel_flow: zdot[b][m] = (z[b][m] - z_prev[b][k]) / dt[b] for the first k with ids_prev[b][k] == ids[b][m] >= 0, where all
// four coordinates are finite and dt[b] > 0; NaN otherwise.  One workgroup of 64 per filter.
__global__ __launch_bounds__(64) void k_pixel_flow(int B, int Mp, const double* __restrict__ z_prev, const int* __restrict__ ids_prev,
                                                   int M, const double* __restrict__ z, const int* __restrict__ ids,
                                                   const double* __restrict__ dt_all, double* __restrict__ zdot) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const double big = 1.7976931348623157e308;
  const double dt = dt_all[b];
  const int* prow = ids_prev + (long)b * Mp;
  for (int i = threadIdx.x; i < M; i += 64) {
    const long at = (long)b * M + i;
    const int id = ids[at];
    double o0 = nan, o1 = nan;
    if (id >= 0 && dt > 0.0) {
      int k = -1;
      for (int j = 0; j < Mp; j++)
        if (prow[j] == id) { k = j; break; }
      if (k >= 0) {
        const double a0 = z[2 * at], a1 = z[2 * at + 1];
        const double p0 = z_prev[2 * ((long)b * Mp + k)], p1 = z_prev[2 * ((long)b * Mp + k) + 1];
        if (fabs(a0) <= big && fabs(a1) <= big && fabs(p0) <= big && fabs(p1) <= big) {   // (false for a NaN)
          o0 = (a0 - p0) / dt;
          o1 = (a1 - p1) / dt;
        }
      }
    }
    zdot[2 * at] = o0;
    zdot[2 * at + 1] = o1;
  }
}

// viekf_frame_intake_pixel_vel: which entries of a frame are PIXEL_VEL measurements, and their slots.  One workgroup of 64 per
// filter.  slot_out [B][M]: the slot of the entry's id in the intake's table; -1 (the update answers SKIPPED) for an entry that
// is no measurement or a filter without a frame; kPixvelNoSlot (>= every len_features: INVALID) for an id that is not in the
// table, and for every id >= 0 of a filter whose table is stale.   act_out [B][M]: use_pixel_vel.
constexpr int kPixvelNoSlot = 0x7fffffff;
__global__ __launch_bounds__(64) void k_frame_pixvel_plan(int B, int N, int M, const int* __restrict__ len, const int* __restrict__ tab,
                                                          const int* __restrict__ tlen, const int* __restrict__ ids,
                                                          const double* __restrict__ zdot, const int* __restrict__ feat_result,
                                                          const unsigned char* __restrict__ active, int use_pixel_vel,
                                                          int* __restrict__ slot_out, unsigned char* __restrict__ act_out) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const bool act = active ? active[b] != 0 : true;
  const int tl = tlen[b];
  const bool stale = len[b] != tl;
  const int* row = tab + (long)b * N;
  const double big = 1.7976931348623157e308;
  for (int i = threadIdx.x; i < M; i += 64) {
    const long at = (long)b * M + i;
    const int id = ids[at];
    int slot = -1;
    if (act && id >= 0) {
      if (stale) slot = kPixvelNoSlot;
      else {
        const int fr = feat_result[at];
        const double d0 = zdot[2 * at], d1 = zdot[2 * at + 1];
        if ((fr == 0 || fr == 1) && fabs(d0) <= big && fabs(d1) <= big) {   // queued as FEAT, finite flow
          slot = kPixvelNoSlot;
          for (int f = 0; f < tl && f < N; f++)
            if (row[f] == id) { slot = f; break; }
        }
      }
    }
    slot_out[at] = slot;
    act_out[at] = use_pixel_vel ? (unsigned char)1 : (unsigned char)0;
  }
}

}  // namespace viekf
