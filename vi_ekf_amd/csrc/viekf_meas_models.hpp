// viekf_meas_models.hpp -- the reference's measurement-model table on the device (src/vi_ekf/vi_ekf_meas.cpp:281-386): the type
// codes, zhat = h(x) with the non-zero columns of H (meas_model), the residual z [-] zhat (meas_residual) and the small dense
// inverse of the innovation covariance.  Shared by the generic update (viekf_kernels_generic.hpp), the read-only evaluations
// (viekf_kernels_hooks.hpp) and the consistency diagnostics (viekf_kernels_diag.hpp).  Device functions only, no __global__.
#pragma once
#include "viekf_device.hpp"

namespace viekf {

constexpr int MT_ACC = 0, MT_ALT = 1, MT_ATT = 2, MT_POS = 3, MT_VEL = 4, MT_QZETA = 5, MT_FEAT = 6, MT_DEPTH = 8,
              MT_INV_DEPTH = 9;   // include/vi_ekf.h:113-124

// r x r inverse (r <= 3) by LU with partial pivoting, row-major (Eigen's dynamic-size inverse, vi_ekf_meas.cpp:232)
__device__ __forceinline__ void small_inverse_dev(int r, const double* S, double* Si) {
  double a[9], b[9];
  for (int i = 0; i < r; i++) for (int j = 0; j < r; j++) { a[i * 3 + j] = S[i * r + j]; b[i * 3 + j] = (i == j) ? 1.0 : 0.0; }
  for (int c = 0; c < r; c++) {
    int piv = c; double best = fabs(a[c * 3 + c]);
    for (int i = c + 1; i < r; i++) if (fabs(a[i * 3 + c]) > best) { best = fabs(a[i * 3 + c]); piv = i; }
    if (piv != c) for (int j = 0; j < r; j++) {
      double t = a[c * 3 + j]; a[c * 3 + j] = a[piv * 3 + j]; a[piv * 3 + j] = t;
      t = b[c * 3 + j]; b[c * 3 + j] = b[piv * 3 + j]; b[piv * 3 + j] = t;
    }
    for (int i = c + 1; i < r; i++) {
      const double l = a[i * 3 + c] / a[c * 3 + c];
      for (int j = 0; j < r; j++) { a[i * 3 + j] -= l * a[c * 3 + j]; b[i * 3 + j] -= l * b[c * 3 + j]; }
    }
  }
  for (int j = 0; j < r; j++)
    for (int i = r - 1; i >= 0; i--) {
      double s = b[i * 3 + j];
      for (int k = i + 1; k < r; k++) s -= a[i * 3 + k] * Si[k * r + j];
      Si[i * r + j] = s / a[i * 3 + i];
    }
}

// the models that measure a feature: they take a feature slot (QZETA, FEAT, DEPTH, INV_DEPTH)
__device__ __forceinline__ bool meas_needs_slot(int type) {
  return type == MT_QZETA || type == MT_FEAT || type == MT_DEPTH || type == MT_INV_DEPTH;
}

// The reference's measurement models (src/vi_ekf/vi_ekf_meas.cpp:281-386): zhat = h(x) and the non-zero columns of H -- at most six
// (`cols`, their number `nc`), Hc [3][6] row-major = the entries of H in those columns.  One lane; xs = the filter's state.
__device__ __forceinline__ void meas_model(int type, const double* xs, int slot, const DevParams& prm, double* zhat, int* cols,
                                           double* Hc, int& nc) {
  nc = 0;
  for (int i = 0; i < 18; i++) Hc[i] = 0.0;
  auto col = [&](int c) { cols[nc] = c; return nc++; };
  if (type == MT_ACC) {                                       // vi_ekf_meas.cpp:281-306
    if (prm.use_drag_term) {
      const double mu = xs[xMU];
      zhat[0] = -mu * xs[xVEL] + xs[xB_A]; zhat[1] = -mu * xs[xVEL + 1] + xs[xB_A + 1];
      int c;
      c = col(dxVEL); Hc[0 * 6 + c] = -mu;  c = col(dxVEL + 1); Hc[1 * 6 + c] = -mu;
      c = col(dxB_A); Hc[0 * 6 + c] = 1.0;  c = col(dxB_A + 1); Hc[1 * 6 + c] = 1.0;
      c = col(dxMU); Hc[0 * 6 + c] = -xs[xVEL]; Hc[1 * 6 + c] = -xs[xVEL + 1];
    } else {
      const double g[3] = {0.0, 0.0, kGravity}; double gB[3], ng[3], Sk[9];
      q_rotp(xs + xATT, g, gB);
      for (int i = 0; i < 3; i++) { zhat[i] = xs[xB_A + i] - gB[i]; ng[i] = -1.0 * gB[i]; }
      skew3(ng, Sk);
      for (int j = 0; j < 3; j++) { const int c = col(dxATT + j); for (int i = 0; i < 3; i++) Hc[i * 6 + c] = Sk[i * 3 + j]; }
      for (int j = 0; j < 3; j++) { const int c = col(dxB_A + j); Hc[j * 6 + c] = 1.0; }
    }
  } else if (type == MT_ALT) { zhat[0] = -xs[xPOS + 2]; const int c = col(dxPOS + 2); Hc[c] = -1.0; }
  else if (type == MT_ATT) { for (int i = 0; i < 4; i++) zhat[i] = xs[xATT + i]; for (int j = 0; j < 3; j++) { const int c = col(dxATT + j); Hc[j * 6 + c] = 1.0; } }
  else if (type == MT_POS) { for (int j = 0; j < 3; j++) { zhat[j] = xs[xPOS + j]; const int c = col(dxPOS + j); Hc[j * 6 + c] = 1.0; } }
  else if (type == MT_VEL) { for (int j = 0; j < 3; j++) { zhat[j] = xs[xVEL + j]; const int c = col(dxVEL + j); Hc[j * 6 + c] = 1.0; } }
  else if (type == MT_QZETA) { for (int i = 0; i < 4; i++) zhat[i] = xs[xZ + 5 * slot + i]; for (int j = 0; j < 2; j++) { const int c = col(dxZ + 3 * slot + j); Hc[j * 6 + c] = 1.0; } }
  else if (type == MT_FEAT) {
    double Hb[4]; h_feat(xs + xZ + 5 * slot, prm, zhat, Hb);
    for (int j = 0; j < 2; j++) { const int c = col(dxZ + 3 * slot + j); Hc[0 * 6 + c] = Hb[0 * 2 + j]; Hc[1 * 6 + c] = Hb[1 * 2 + j]; }
  } else if (type == MT_DEPTH) { const double rho = xs[xZ + 5 * slot + 4]; zhat[0] = 1.0 / rho; const int c = col(dxZ + 3 * slot + 2); Hc[c] = -1.0 / (rho * rho); }
  else if (type == MT_INV_DEPTH) { zhat[0] = xs[xZ + 5 * slot + 4]; const int c = col(dxZ + 3 * slot + 2); Hc[c] = 1.0; }
}

// residual z [-] zhat of a model (vi_ekf_meas.cpp:209-220): a quaternion measurement by its boxminus, the others subtract
__device__ __forceinline__ void meas_residual(int type, const double* z, const double* zhat, int zdim, double* r3) {
  if (type == MT_QZETA) q_feat_boxminus_dev(z, zhat, r3);           // :210-213
  else if (type == MT_ATT) q_boxminus_dev(z, zhat, r3);             // :214-217
  else for (int i = 0; i < zdim && i < 3; i++) r3[i] = z[i] - zhat[i];
}

}  // namespace viekf
