// viekf_kernels_lifecycle.hpp -- the kernels that change which features a filter holds and where its frame sits: init_feature,
// keep_only_features / clear_feature, the keyframe reset and the reset to the initial state.  Defines kernels: included from
// viekf_dispatch.hpp only.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_stream_lds.hpp"

namespace viekf {

// ------------------------------------------------------------------------------------------------
// init_feature (vi_ekf_feat.cpp:6-47), one workgroup per filter
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_init_feature(StreamArgs a, const double* __restrict__ pix_all,
                                                    const double* __restrict__ depth_all,
                                                    const unsigned char* __restrict__ mask, int* __restrict__ ok) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  if (mask && !mask[b]) { if (ok && tid == 0) ok[b] = 0; return; }
  const int len = a.len[b];
  if (len >= a.N) { if (ok && tid == 0) ok[b] = 0; return; }   // :9-10
  const int n = a.n, ld = a.ld;
  double* P = a.P + a.si(b) * n * ld;
  const int d0 = 16 + 3 * len, dmax = d0 + 3;
  if (tid == 0) {
    double q[4], rho;
    init_feature_state(pix_all + 2L * b, depth_all ? depth_all[b] : NAN, a.prm(b), q, &rho);
    double* xf = a.x + a.si(b) * a.nxs + xZ + 5 * len;
    xf[0] = q[0]; xf[1] = q[1]; xf[2] = q[2]; xf[3] = q[3]; xf[4] = rho;
  }
  // zero the cross strips, set the 3x3 block to P0_feat (:39-42)
  for (int e = tid; e < 3 * d0; e += T) {
    const int j = e / 3, r = e % 3;
    P[(d0 + r) + (long)j * ld] = 0.0;
    P[j + (long)(d0 + r) * ld] = 0.0;
  }
  if (tid < 9) {
    const int r = tid % 3, c = tid / 3;
    P[(d0 + r) + (long)(d0 + c) * ld] = (r == c) ? a.prm(b).P0_feat[r] : 0.0;
  }
  (void)dmax;
  __syncthreads();
  if (tid == 0) {
    a.len[b] = len + 1;
    if (ok) ok[b] = 1;
  }
}

// ------------------------------------------------------------------------------------------------
// keep_only_features / clear_feature (vi_ekf_feat.cpp:50-73,81-117): drop the features whose keep flag is 0 and shift the
// survivors (state and covariance rows/columns) to the upper-left corner, zeroing what is left over.  One workgroup per
// filter; columns are moved through an LDS buffer in increasing order, so the in-place compaction never overwrites a
// column that is still needed.  (The keyframe-overlap bookkeeping of keep_only_features stays on the host.)
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_keep_features(StreamArgs a, const unsigned char* __restrict__ keep_all,
                                                     int* __restrict__ new_len) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n, ld = a.ld, N = a.N;
  const KeepLds lds(n);
  char* base = reinterpret_cast<char*>(smem);
  double* colbuf = reinterpret_cast<double*>(base + lds.colbuf);   // [n]
  int* srcrow = reinterpret_cast<int*>(base + lds.srcrow);         // [n] old row index of new row i (or -1)
  int* cnt = reinterpret_cast<int*>(base + lds.cnt);
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const unsigned char* keep = keep_all + (long)b * N;
  if (tid == 0) {
    for (int i = 0; i < 16; i++) srcrow[i] = i;
    int k = 0;
    for (int f = 0; f < len; f++)
      if (keep[f]) { for (int q = 0; q < 3; q++) srcrow[16 + 3 * k + q] = 16 + 3 * f + q; k++; }
    for (int i = 16 + 3 * k; i < n; i++) srcrow[i] = -1;
    *cnt = k;
  }
  __syncthreads();
  const int k = *cnt;
  if (k == len) { if (new_len && tid == 0) new_len[b] = len; return; }   // nothing to drop
  // state: features are 5 doubles each
  if (tid == 0) {
    int w = 0;
    for (int f = 0; f < len; f++)
      if (keep[f]) { if (w != f) for (int q = 0; q < 5; q++) xg[xZ + 5 * w + q] = xg[xZ + 5 * f + q]; w++; }
    for (int i = xZ + 5 * k; i < xZ + 5 * N; i++) xg[i] = 0.0;   // "clean up the rest" (vi_ekf_feat.cpp:66-69): EVERYTHING past the
  }                                                              // kept features, also what a replay from older history left there
  const int nk = 16 + 3 * k, nold = n;
  for (int jn = 0; jn < nold; jn++) {
    const int jo = (jn < nk) ? srcrow[jn] : -1;
    if (jo >= 0) for (int i = tid; i < nk; i += T) colbuf[i] = P[srcrow[i] + (long)jo * ld];
    __syncthreads();
    for (int i = tid; i < nold; i += T) P[i + (long)jn * ld] = (jo >= 0 && i < nk) ? colbuf[i] : 0.0;
    __syncthreads();
  }
  if (tid == 0) { a.len[b] = k; if (new_len) new_len[b] = k; }
}

// ------------------------------------------------------------------------------------------------
// keyframe reset ("Dan's way", vi_ekf_kfr.cpp:56-157): position <- 0, yaw <- 0, P <- N P N^T where N differs from I only
// in the position block (0) and the attitude block (RMEKF Eq. 81).  One workgroup per filter, in place: first the row
// operation N P (every thread owns columns), then the column operation (every thread owns rows).  edge [B][17] (optional):
// {t(3), q_yaw(4), cov_pos(9, column-major), cov_yaw} of the relative pose before the reset, for the caller's global-pose
// bookkeeping (:58-62,125-126,147-149 -- the Xformd algebra of the reference's `geometry` dependency stays with the caller).
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T) void k_keyframe_reset(StreamArgs a, const unsigned char* __restrict__ mask,
                                                      double* __restrict__ edge_all) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  if (mask && !mask[b]) return;
  const int n = a.n, ld = a.ld;
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const double* q = xg + xATT;
  const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double yaw = q_yaw_dev(q);
  const double roll = atan2(2.0 * (qw * qx + qy * qz), 1.0 - 2.0 * (qx * qx + qy * qy));    // :211-214
  const double pitch = asin(2.0 * (qw * qy - qz * qx));                                     // :216-219
  const double cp = cos(roll), sp = sin(roll), tt = tan(pitch);                             // vi_ekf_kfr.cpp:134-136
  const double Na[9] = {1.0, sp * tt, cp * tt, 0.0, cp * cp, -cp * sp, 0.0, -cp * sp, sp * sp};   // row-major (:139-142)
  if (edge_all && tid == 0) {
    double* e = edge_all + (long)b * 17;
    for (int i = 0; i < 3; i++) e[i] = xg[xPOS + i];
    q_from_yaw_dev(yaw, e + 3);
    for (int j = 0; j < 3; j++)
      for (int i = 0; i < 3; i++) e[7 + i + 3 * j] = P[(dxPOS + i) + (long)(dxPOS + j) * ld];
    e[16] = P[(dxATT + 2) + (long)(dxATT + 2) * ld];
  }
  __syncthreads();   // (the edge reads P and x before they change)
  // rows: T = N P
  for (int j = tid; j < n; j += T) {
    double* c = P + (long)j * ld;
    const double a0 = c[dxATT], a1 = c[dxATT + 1], a2 = c[dxATT + 2];
    c[dxATT] = Na[0] * a0 + Na[1] * a1 + Na[2] * a2;
    c[dxATT + 1] = Na[3] * a0 + Na[4] * a1 + Na[5] * a2;
    c[dxATT + 2] = Na[6] * a0 + Na[7] * a1 + Na[8] * a2;
    c[dxPOS] = 0.0; c[dxPOS + 1] = 0.0; c[dxPOS + 2] = 0.0;
  }
  __syncthreads();
  // columns: P = T N^T
  for (int i = tid; i < n; i += T) {
    const double a0 = P[i + (long)dxATT * ld], a1 = P[i + (long)(dxATT + 1) * ld], a2 = P[i + (long)(dxATT + 2) * ld];
    P[i + (long)dxATT * ld] = a0 * Na[0] + a1 * Na[1] + a2 * Na[2];
    P[i + (long)(dxATT + 1) * ld] = a0 * Na[3] + a1 * Na[4] + a2 * Na[5];
    P[i + (long)(dxATT + 2) * ld] = a0 * Na[6] + a1 * Na[7] + a2 * Na[8];
    P[i + (long)dxPOS * ld] = 0.0; P[i + (long)(dxPOS + 1) * ld] = 0.0; P[i + (long)(dxPOS + 2) * ld] = 0.0;
  }
  __syncthreads();
  // N P N^T of a symmetric P is symmetric; make it so bit for bit (the update kernels rely on it): the attitude rows take
  // the values of the attitude columns
  for (int i = tid; i < n; i += T)
    for (int c = 0; c < 3; c++)
      if (i < dxATT || i > dxATT + c) P[(dxATT + c) + (long)i * ld] = P[i + (long)(dxATT + c) * ld];
  if (tid == 0) {
    const double cr = cos(roll / 2.0), ct = cos(pitch / 2.0), sr = sin(roll / 2.0), st = sin(pitch / 2.0);
    xg[xPOS] = 0.0; xg[xPOS + 1] = 0.0; xg[xPOS + 2] = 0.0;                                  // :65
    xg[xATT] = cr * ct; xg[xATT + 1] = sr * ct; xg[xATT + 2] = cr * st; xg[xATT + 3] = -sr * st;   // from_euler(roll,pitch,0)
  }
}

// fill every filter with the initial state (vi_ekf.cpp:70-81 / :134-144)
// x0 / Pdiag: one set (strides 0) or filter b's own at b * stride
__global__ void k_reset(StreamArgs a, const double* __restrict__ x0 /*17*/, const double* __restrict__ Pdiag /*n*/, long x0_stride,
                        long pd_stride) {
  const int b = blockIdx.x;
  if (b >= a.B) return;
  x0 += b * x0_stride; Pdiag += b * pd_stride;
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * a.n * a.ld;
  for (int i = threadIdx.x; i < a.nxs; i += blockDim.x) xg[i] = (i < 17) ? x0[i] : 0.0;
  const long tot = (long)a.n * a.ld;
  for (long e = threadIdx.x; e < tot; e += blockDim.x) {
    const int i = (int)(e % a.ld), j = (int)(e / a.ld);
    P[e] = (i == j) ? Pdiag[i] : 0.0;
  }
  if (threadIdx.x == 0) { a.len[b] = 0; a.flags[b] = 0; }
}

}  // namespace viekf
