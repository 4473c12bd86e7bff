// viekf_pixvel_model.hpp -- the PIXEL_VEL measurement model, the one row of the reference's table its authors left empty
// (h_pixel_vel, src/vi_ekf/vi_ekf_meas.cpp:388-395 is a TODO): the image velocity of a tracked feature, stated once for the
// read-only evaluation and the update kernel (viekf_kernels_pixvel.hpp).  Device functions only, no __global__.
//
//   zhat = Hb(q_zeta) f_zeta(x, g)   [px / s]
// Hb = the 2x2 block of h_feat (d pixel / d delta, delta the boxplus perturbation of q_zeta), f_zeta = -T^T (omega_c + rho zeta x v_c)
// the first two outputs of feature_dynamics at omega = g_b - b_g (g_b: the raw gyro sample rotated by q_b_u, as the propagate
// rotates it); the accelerometer does not enter.  Exact to first order by the definition of Hb: the pixel is h_feat(q_zeta(t))
// and q_zeta moves by f_zeta dt under boxplus.
//
// H has nine non-zero columns: VEL (3), B_G (3), the bearing (2) and rho (1).
//   VEL, B_G, rho: Hb times the plain partials of f_zeta, which are the blocks Afv, Afg and Aff[:, 2] of feature_dynamics.
//   The bearing: with w = omega_c + rho zeta x v_c and T T^T = I - zeta zeta^T the bearing vector moves by
//     zeta_dot = (T f_zeta) x zeta = zeta x w = g(zeta),   g = zeta x omega_c + rho (zeta (zeta . v_c) - v_c),
//   so zhat = Jpi(zeta) g(zeta), Jpi = (1 / e_z) F (I - zeta e_z^T / e_z) the Jacobian of the projection, depends on q_zeta
//   through zeta alone (not on the roll about it), and d zeta / d delta = -skew(zeta) T (what Hb = Jpi (-skew(zeta) T) uses):
//     d zhat / d delta = D (-skew(zeta) T),   D = d (Jpi g) / d zeta   (2 x 3, zeta taken as free in R^3),
//     D_r = F_r [ dg_r / e_z - g_r e_z^T / e_z^2 - e_r^T g_z / e_z^2 - zeta_r dg_z / e_z^2 + 2 zeta_r g_z e_z^T / e_z^3 ],
//     dg = d g / d zeta = -skew(omega_c) + rho ((zeta . v_c) I + zeta v_c^T).
//   (Aff's own 2x2 block is NOT this: A is the error-state dynamics and carries the frame-transport term.)
// Every column of the numpy restatement (tests/pixvel_ref.py) is checked against central differences over boxplus in
// tests/test_pixvel_ref_cpu.py; tests/test_gpu_pixvel.py holds this code to that restatement at the parity tolerance.
#pragma once
#include "viekf_device.hpp"

namespace viekf {

constexpr int kPixvelCols = 9;   // VEL 3, B_G 3, bearing 2, rho 1

// the columns of H for the feature in `slot`, in the order of Hc's columns
__device__ __forceinline__ void pixel_vel_cols(int slot, int* cols) {
  for (int j = 0; j < 3; j++) { cols[j] = dxVEL + j; cols[3 + j] = dxB_G + j; cols[6 + j] = dxZ + 3 * slot + j; }
}

// the body-frame input of a raw gyro sample: rotated by q_b_u (vi_ekf.cpp:265-267), no accelerometer
__device__ __forceinline__ void pixel_vel_input(const DevParams& prm, const double* gyro, double* ub) {
  ub[0] = ub[1] = ub[2] = 0.0;
  q_rota(prm.q_b_u, gyro, ub + 3);
}

// zhat [2] and Hc [2][9] row-major (columns as pixel_vel_cols) at the state xs, for the feature in `slot` and the raw gyro sample.
// One lane.
__device__ __forceinline__ void pixel_vel_model(const double* xs, int slot, const double* gyro, const DevParams& prm, double* zhat, double* Hc) {
  double ub[6];
  pixel_vel_input(prm, gyro, ub);
  BodyCtx c;
  body_ctx(xs, ub, prm, c);
  const double* qz = xs + xZ + 5 * slot;
  const double rho = qz[4];
  double f3[3], Afv[9], Afg[9], Aff[9], pix[2], Hb[4];
  feature_dynamics(qz, rho, c, f3, Afv, Afg, Aff);
  h_feat(qz, prm, pix, Hb);
  double t1[3], t2[3], z[3];
  bearing_frame(qz, t1, t2, z);
  // g and dg / d zeta
  double zxw[3], g[3], dg[9], skw[9];
  cross3(z, c.omega_c, zxw);
  const double zv = dot3(z, c.vel_c);
  skew3(c.omega_c, skw);
  for (int i = 0; i < 3; i++) {
    g[i] = zxw[i] + rho * (z[i] * zv - c.vel_c[i]);
    for (int j = 0; j < 3; j++) dg[i * 3 + j] = -skw[i * 3 + j] + rho * ((i == j ? zv : 0.0) + z[i] * c.vel_c[j]);
  }
  const double ez = z[2], ez2 = ez * ez, ez3 = ez2 * ez;
  // -skew(zeta) T: its columns are t_k x zeta
  double d1[3], d2[3];
  cross3(t1, z, d1);
  cross3(t2, z, d2);
  for (int r = 0; r < 2; r++) {
    zhat[r] = Hb[r * 2 + 0] * f3[0] + Hb[r * 2 + 1] * f3[1];
    for (int j = 0; j < 3; j++) {
      Hc[r * 9 + j] = Hb[r * 2 + 0] * Afv[0 * 3 + j] + Hb[r * 2 + 1] * Afv[1 * 3 + j];
      Hc[r * 9 + 3 + j] = Hb[r * 2 + 0] * Afg[0 * 3 + j] + Hb[r * 2 + 1] * Afg[1 * 3 + j];
    }
    Hc[r * 9 + 8] = Hb[r * 2 + 0] * Aff[0 * 3 + 2] + Hb[r * 2 + 1] * Aff[1 * 3 + 2];
    double D[3];
    for (int j = 0; j < 3; j++) D[j] = dg[r * 3 + j] / ez - z[r] * dg[2 * 3 + j] / ez2;
    D[2] += -g[r] / ez2 + 2.0 * z[r] * g[2] / ez3;
    D[r] += -g[2] / ez2;
    for (int j = 0; j < 3; j++) D[j] *= prm.focal[r];
    Hc[r * 9 + 6] = dot3(D, d1);
    Hc[r * 9 + 7] = dot3(D, d2);
  }
}

}  // namespace viekf
