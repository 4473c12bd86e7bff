// viekf_rec_align.hpp -- the alignment of the flight recorder's trajectory error (include/viekf_rec.h): from
// the 3x3 matrix A = sum (p_t - c_t)(p_e - c_e)^T to the quaternion q_a with q_a.rota(v) = R_a v.  Plain arithmetic on a
// handful of doubles, for host and device alike: k_rec_trajectory (viekf_kernels_rec.hpp) calls it on the device, and
// tests/cpp/rec_align_model.cpp compiles it with a plain C++ compiler and holds it against known rotations.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define REC_HD __host__ __device__ __forceinline__
#else
#define REC_HD inline
#endif

namespace viekf {

// Sweeps of the cyclic Jacobi iteration on Horn's 4x4 matrix.  The iteration converges quadratically once the off-diagonal
// part is small; tests/cpp/rec_align_model.cpp measures, over 20000 matrices A (random, rank-deficient, and scaled between
// 1e-12 and 1e+12), the off-diagonal norm relative to the matrix norm after every sweep: at most 4.4e-2 after 3, 1.5e-5
// after 4, 3.9e-17 after 5, and what rounding refills (1e-17) from there.  Seven leaves two sweeps in hand; a sweep is six
// rotations of a few dozen flops, once per filter and call.
constexpr int kRecJacobiSweeps = 7;

// yaw and translation: the rotation about z that maximises tr(R A^T)
REC_HD void rec_align_yaw(const double* A, double* q) {
  const double s = A[3] - A[1], c = A[0] + A[4];
  const double th = (s == 0.0 && c == 0.0) ? 0.0 : atan2(s, c);
  q[0] = cos(0.5 * th); q[1] = 0.0; q[2] = 0.0; q[3] = sin(0.5 * th);
}

// One Jacobi rotation in the (P, Q) plane of the symmetric 4x4 matrix N (full storage, both triangles kept equal) with the
// eigenvector matrix V (columns).  The indices are template arguments so that N and V stay in registers.
template <int P, int Q>
REC_HD void rec_jacobi_rotate(double (&N)[4][4], double (&V)[4][4]) {
  const double apq = N[P][Q];
  if (apq == 0.0) return;
  const double tau = (N[Q][Q] - N[P][P]) / (2.0 * apq);
  const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));   // the smaller root: |angle| <= pi/4
  const double c = 1.0 / sqrt(1.0 + t * t), s = t * c;
#pragma unroll
  for (int k = 0; k < 4; k++) {   // columns P and Q
    const double kp = N[k][P], kq = N[k][Q];
    N[k][P] = c * kp - s * kq;
    N[k][Q] = s * kp + c * kq;
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {   // rows P and Q
    const double pk = N[P][k], qk = N[Q][k];
    N[P][k] = c * pk - s * qk;
    N[Q][k] = s * pk + c * qk;
  }
  N[P][Q] = 0.0; N[Q][P] = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const double kp = V[k][P], kq = V[k][Q];
    V[k][P] = c * kp - s * kq;
    V[k][Q] = s * kp + c * kq;
  }
}

// `sweeps` cyclic sweeps; returns the off-diagonal Frobenius norm that is left (the model program reads it)
REC_HD double rec_jacobi4(double (&N)[4][4], double (&V)[4][4], int sweeps) {
#pragma unroll
  for (int i = 0; i < 4; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
  for (int s = 0; s < sweeps; s++) {
    rec_jacobi_rotate<0, 1>(N, V); rec_jacobi_rotate<0, 2>(N, V); rec_jacobi_rotate<0, 3>(N, V);
    rec_jacobi_rotate<1, 2>(N, V); rec_jacobi_rotate<1, 3>(N, V); rec_jacobi_rotate<2, 3>(N, V);
  }
  return sqrt(2.0 * (N[0][1] * N[0][1] + N[0][2] * N[0][2] + N[0][3] * N[0][3] + N[1][2] * N[1][2] + N[1][3] * N[1][3] + N[2][3] * N[2][3]));
}

// Horn's symmetric 4x4 matrix of A (row-major 3x3, A = sum t e^T: the rotation takes e to t)
REC_HD void rec_horn_matrix(const double* A, double (&N)[4][4]) {
  // S = A^T in Horn's notation (S_xy = sum e_x t_y)
  const double Sxx = A[0], Sxy = A[3], Sxz = A[6], Syx = A[1], Syy = A[4], Syz = A[7], Szx = A[2], Szy = A[5], Szz = A[8];
  N[0][0] = Sxx + Syy + Szz; N[0][1] = Syz - Szy;       N[0][2] = Szx - Sxz;        N[0][3] = Sxy - Syx;
  N[1][1] = Sxx - Syy - Szz; N[1][2] = Sxy + Syx;       N[1][3] = Szx + Sxz;
  N[2][2] = -Sxx + Syy - Szz; N[2][3] = Syz + Szy;
  N[3][3] = -Sxx - Syy + Szz;
  N[1][0] = N[0][1]; N[2][0] = N[0][2]; N[3][0] = N[0][3]; N[2][1] = N[1][2]; N[3][1] = N[1][3]; N[3][2] = N[2][3];
}

// SE(3) without scale: q = the unit eigenvector of the largest eigenvalue of Horn's matrix, w >= 0.  Of equal eigenvalues the
// first in the order of the diagonal is taken (A = 0, one frame: the identity).
REC_HD void rec_align_se3(const double* A, double* q) {
  double N[4][4], V[4][4];
  rec_horn_matrix(A, N);
  rec_jacobi4(N, V, kRecJacobiSweeps);
  double best = N[0][0];
  double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
  for (int j = 1; j < 4; j++) {
    const bool take = N[j][j] > best;
    best = take ? N[j][j] : best;
    v0 = take ? V[0][j] : v0; v1 = take ? V[1][j] : v1; v2 = take ? V[2][j] : v2; v3 = take ? V[3][j] : v3;
  }
  const double nrm = sqrt(v0 * v0 + v1 * v1 + v2 * v2 + v3 * v3);
  const double sc = (v0 < 0.0 ? -1.0 : 1.0) / nrm;
  q[0] = v0 * sc; q[1] = v1 * sc; q[2] = v2 * sc; q[3] = v3 * sc;
}

}  // namespace viekf
