// viekf_kernels_pixvel.hpp -- the PIXEL_VEL measurement (viekf_pixvel_model.hpp): the update kernel, one entry per launch, the
// read-only evaluation and the flow of a frame's features by id.  (The id -> slot lookup of the intake's pixel-velocity step:
// k_frame_slot_plan, viekf_kernels_frame.hpp.)
// Defines kernels: included from viekf_dispatch.hpp only.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"
#include "viekf_onepass.hpp"
#include "viekf_pixvel_lds.hpp"
#include "viekf_pixvel_model.hpp"

namespace viekf {

// The arithmetic both routes share is viekf_onepass.hpp's at rank 2, stated once so that they contract alike: route 1 must
// give route 0's bits.  Route 0 keeps W and K interleaved, so it hands the pairs over by value:
//   a gain element K[i][q];  one element of the correction;  one applied entry's downdate of one element.
__device__ __forceinline__ double pixvel_gain(double w0, double w1, const double* Si, int q) {
  const double w[2] = {w0, w1};
  return onepass_gain<2>(w, Si, q);
}
__device__ __forceinline__ double pixvel_dx(double l, double k0, double k1, double r0, double r1) {
  const double k[2] = {k0, k1}, r[2] = {r0, r1};
  return onepass_dx<2>(l, k, r);
}
__device__ __forceinline__ double pixvel_downdate(double v, double L, double k0, double k1, double w0, double w1) {
  const double k[2] = {k0, k1}, w[2] = {w0, w1};
  return onepass_downdate<2>(v, L, k, w);
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
  const DevParams& prm = a.prm(b);
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
  for (int i = tid; i < n; i += T) lam[i] = a.lam(b)[i];
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
        P[at] = pixvel_downdate(P[at], partial_L(partial, lam[i], lj), K[2 * hi], K[2 * hi + 1], W[2 * lo], W[2 * lo + 1]);
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
// left-looking (onepass_rebuild<2>): the start P's column, from global memory, which nobody writes before the trailing pass,
// minus the downdates of the entries applied so far, which their W and S^-1 in LDS give.  The rho diagonals in D, the
// trailing pass and what is never touched: viekf_onepass.hpp.
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
  const DevParams& prm = a.prm(b);
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
  const bool partial = prm.use_partial_update != 0;
  const long row = (long)b * M;
  const double* gyro = gyro_all + 3L * b;
  const bool gyro_nan = gyro[0] != gyro[0] || gyro[1] != gyro[1] || gyro[2] != gyro[2];
  auto entry_of = [&](int e) { return order ? M - 1 - e : e; };
  auto p_low = [&](int i, int c) { return (i >= c) ? P[i + (long)c * ld] : P[c + (long)i * ld]; };   // (the lower triangle only)
  const int bcol[6] = {dxVEL, dxVEL + 1, dxVEL + 2, dxB_G, dxB_G + 1, dxB_G + 2};

  onepass_load<T>(a, b, xg, P, len, xs, lam, D);
  for (int i = tid; i < nact; i += T) {
    double v[6];
#pragma unroll
    for (int j = 0; j < 6; j++) v[j] = p_low(i, bcol[j]);
#pragma unroll
    for (int j = 0; j < 6; j++) Pb[j * nW + i] = v[j];
  }

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
      for (int f = tid; f < len; f += T) fix_depth_diag(xs, D, f, prm, flag);
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
      const double L = partial_L(partial, lam[i], lam[c]);
      v = onepass_rebuild<2, 1>(v, L, Wall, nW, Sinv, napp, hi, lo);
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
        Pb[j * nW + i] = onepass_apply<2>(Pb[j * nW + i], partial_L(partial, lam[i], lam[c]), W0, nW, Si, max(i, c), min(i, c));
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
        D[f] = onepass_apply<2>(D[f], partial_L(partial, lam[dr], lam[dr]), W0, nW, Si, dr, dr);
      }
      fix_depth_diag(xs, D, f, prm, flag);
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
  onepass_store<T>(a, b, xg, P, len, napp, flag, xs, D);
  if (napp == 0) return;
  onepass_trailing<T, 2>(P, ld, nact, nW, napp, partial, Wall, Sinv, lam);
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
    pixel_vel_model(xs, slot, gyro_all + 3L * b, a.prm(b), zhat, Hc);
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

}  // namespace viekf
