// viekf_kernels_generic.hpp -- the generic measurement update, for every model of the reference's table but the hot-path FEAT
// loop.  Defines a kernel: included from viekf_dispatch.hpp only.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"
#include "viekf_stream_lds.hpp"

namespace viekf {

// ------------------------------------------------------------------------------------------------
// generic measurement update: VIEKF::update for every measurement model of the reference's table
// (vi_ekf_meas.cpp:196-278 with h_acc/h_alt/h_att/h_pos/h_vel/h_qzeta/h_feat/h_depth/h_inv_depth, :281-386).
// Each H has at most 6 non-zero columns, so W = P H^T is a combination of <= 6 columns of P and the update is the same
// rank-r sweep  P_ij -= Lambda_ij (K_i . W_j)  as for FEAT.  One workgroup per filter, P in HBM/L2 (these models run at
// IMU / truth rate, one per propagate -- not the N-per-frame hot loop).
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_update_generic(StreamArgs a, int type, int zdim, int rdim,
                                                      const double* __restrict__ z_all, const int* __restrict__ slot_all,
                                                      const double* __restrict__ R_all, long r_stride_b,
                                                      const unsigned char* __restrict__ active_all,
                                                      int* __restrict__ result_all) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n, ld = a.ld;
  const DevParams& prm = a.prm(b);
  const GenLds lds(a.nxs, n);
  double* xs = smem + lds.xs;     // [nxs]
  double* W = smem + lds.W;       // [n][3]
  double* K = smem + lds.K;       // [n][3]
  double* lam = smem + lds.lam;   // [n]
  double* sm = smem + lds.sm;     // [64]: hcols (int as double) [0..5], Hc [6..23] (3 rows x 6 cols), res [24..26], ncol [27], Si [28..36], verdict [37]
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const int slot = slot_all ? slot_all[b] : 0;
  const bool active = active_all ? active_all[b] != 0 : true;
  int* res_out = result_all ? &result_all[b] : nullptr;
  if (active_all && active_all[b] == 2) { if (res_out && tid == 0) *res_out = -1; return; }   // this filter skips the call
  unsigned flag = 0;
  if (meas_needs_slot(type) && (slot < 0 || slot >= len)) { if (res_out && tid == 0) *res_out = (slot < 0) ? -1 : 3; return; }
  const double* z = z_all + (long)b * zdim;
  {
    bool isnan_ = false;
    for (int i = 0; i < zdim; i++) isnan_ |= z[i] != z[i];
    if (isnan_) { if (res_out && tid == 0) *res_out = 2; return; }   // MEAS_NAN
  }
  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lam(b)[i];
  __syncthreads();

  if (tid == 0) {   // measurement model: zhat, the non-zero columns of H, residual
    int cols[6]; double Hc[18]; int nc = 0; double zhat[4] = {0, 0, 0, 0}; double r3[3] = {0, 0, 0};
    meas_model(type, xs, slot, prm, zhat, cols, Hc, nc);
    meas_residual(type, z, zhat, zdim, r3);
    for (int i = 0; i < 6; i++) sm[i] = (i < nc) ? (double)cols[i] : 0.0;
    for (int i = 0; i < 18; i++) sm[6 + i] = Hc[i];
    sm[24] = r3[0]; sm[25] = r3[1]; sm[26] = r3[2]; sm[27] = (double)nc;
  }
  __syncthreads();
  if (!active) {   // :230 -- an inactive measurement only runs fix_depth (and the logger)
    for (int f = tid; f < len; f += T) fix_depth_one(xs, P, ld, f, prm, flag);
    __syncthreads();
    for (int i = tid; i < xZ + 5 * len; i += T) xg[i] = xs[i];
    if (res_out && tid == 0) *res_out = 0;
    if (flag) atomicOr(&a.flags[b], flag);
    return;
  }
  const int nc = (int)sm[27];
  // W = P H^T  (n x r): combination of the nc non-zero columns
  for (int i = tid; i < nact; i += T) {
    double w[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < nc; c++) {
      const double pv = P[i + (long)((int)sm[c]) * ld];
      for (int q = 0; q < rdim; q++) w[q] += pv * sm[6 + q * 6 + c];
    }
    for (int q = 0; q < 3; q++) W[3 * i + q] = w[q];
  }
  __syncthreads();
  if (tid == 0) {   // S = H W[cols] + R, inverse, gate
    const double* R = R_all + (long)b * r_stride_b;   // column-major rdim x rdim
    double S[9], Si[9];
    for (int p = 0; p < rdim; p++)
      for (int q = 0; q < rdim; q++) {
        double s = 0.0;
        for (int c = 0; c < nc; c++) s += sm[6 + p * 6 + c] * W[3 * (int)sm[c] + q];
        S[p * rdim + q] = s + R[p + q * rdim];
      }
    small_inverse_dev(rdim, S, Si);
    double mahal = 0.0;
    for (int q = 0; q < rdim; q++) { double t = 0.0; for (int p = 0; p < rdim; p++) t += sm[24 + p] * Si[p * rdim + q]; mahal += t * sm[24 + q]; }
    for (int i = 0; i < 9; i++) sm[28 + i] = (i < rdim * rdim) ? Si[i] : 0.0;
    sm[37] = (mahal > kGateMahal) ? 1.0 : 0.0;   // :234-239
  }
  __syncthreads();
  if (sm[37] != 0.0) { if (res_out && tid == 0) *res_out = 1; return; }   // gated: returns before fix_depth
  int bad = 0;
  for (int i = tid; i < nact; i += T) {
    for (int q = 0; q < 3; q++) {
      double k = 0.0;
      if (q < rdim) for (int p = 0; p < rdim; p++) k += W[3 * i + p] * sm[28 + p * rdim + q];
      K[3 * i + q] = k;
      if (k != k) bad = 1;
    }
  }
  for (int i = 0; i < 18; i++) if (sm[6 + i] != sm[6 + i]) bad = 1;
  bad = __syncthreads_or(bad);
  if (!bad) {
    const bool partial = prm.use_partial_update != 0;
    if (tid == 0) {
      double dxb[16], xo[17];
      for (int i = 0; i < 16; i++) {
        const double l = partial ? lam[i] : 1.0;
        double s = 0.0;
        for (int q = 0; q < rdim; q++) s += (l * K[3 * i + q]) * sm[24 + q];
        dxb[i] = s;
      }
      body_boxplus(xs, dxb, xo);
      for (int i = 0; i < 17; i++) xs[i] = xo[i];
    }
    for (int f = tid; f < len; f += T) {
      const int d = 16 + 3 * f;
      double dv[3];
      for (int e = 0; e < 3; e++) {
        const double l = partial ? lam[d + e] : 1.0;
        double s = 0.0;
        for (int q = 0; q < rdim; q++) s += (l * K[3 * (d + e) + q]) * sm[24 + q];
        dv[e] = s;
      }
      double qn[4];
      q_feat_boxplus(xs + xZ + 5 * f, dv[0], dv[1], qn);
      double* xf = xs + xZ + 5 * f;
      xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
      xf[4] += dv[2];
    }
    const long tot = (long)nact * nact;
    for (long e = tid; e < tot; e += T) {
      const int i = (int)(e % nact), j = (int)(e / nact);
      const int hi = max(i, j), lo = min(i, j);   // (exactly symmetric result, see k_update_feat_stream)
      double t = 0.0;
      for (int q = 0; q < rdim; q++) t += K[3 * hi + q] * W[3 * lo + q];
      const double li = lam[i], lj = lam[j];
      const double L = partial ? (lj + li - li * lj) : 1.0;
      P[i + (long)j * ld] -= L * t;
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
  if (res_out && tid == 0) *res_out = 0;
  if (flag) atomicOr(&a.flags[b], flag);
}

}  // namespace viekf
