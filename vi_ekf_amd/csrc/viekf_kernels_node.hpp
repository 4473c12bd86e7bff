// viekf_kernels_node.hpp -- the device-resident node graph (include/viekf_node.h): the global pose and
// covariance of every filter across keyframe resets -- the tail of VIEKF::keyframe_reset (reference
// src/vi_ekf/vi_ekf_kfr.cpp:147-150), get_global_pose (:14-21), get_global_cov / propagate_global_covariance (:23-53) -- with
// node, node covariance, true node, reset count and the keyframe trail in device memory.
//
//   k_node_update          one lane per filter: node_cov += Adj(node)^T C Adj(node), the trail entry, node = node * edge, the
//                          true node.  A filter that did not reset is not touched.
//   k_node_global          one lane per filter: pose = node * {x[POS], x[ATT]}, cov = node_cov + Adj(node)^T Cx Adj(node).
//                          READ-ONLY on the batch.  Cx comes from 21 elements of P's lower triangle, each read at an offset
//                          the host chose for the form the live P is in (NodeOffs): the kernel does not know the forms.
//   k_node_global_error    the same pose and covariance, then the 6-dof error against a truth in the inertial frame and its
//                          NEES through a 6x6 Cholesky factorisation in registers.
//   k_node_relative_truth  one wave64 per filter: the truth's columns copied lane-strided, position and attitude by lane 0.
// The work per filter is a few 3x3 products, so the kernels are as plain as that: fp64 throughout, no LDS, no barrier, no
// synchronisation between waves, every loop unrolled over constant bounds so that the small matrices stay in registers (no
// scratch).  Lane -> work: ONE LANE PER FILTER, all 21 loads of P issued before the first use (DESIGN.md §13 says why).
#pragma once
#include "viekf_kernel_args.hpp"

namespace viekf {

// the node graph's device tables, all [B] rows
struct NodeTabs {
  double* node;      // [B][7]
  double* cov;       // [B][36] column-major
  double* tnode;     // [B][7]
  int* count;        // [B]
  double* tr_node;   // [B][cap][7]
  double* tr_edge;   // [B][cap][17]
  int cap;
};

// Offsets, in doubles from a filter's P, of the 21 elements (i, j), i >= j, of the [POS,ATT] x [POS,ATT] block in the order
// k = i (i + 1) / 2 + j (i, j index {POS, POS+1, POS+2, ATT, ATT+1, ATT+2}).  Built by the host (node_offsets, viekf_capi.hip).
struct NodeOffs { int o[21]; };

// ---- 3x3 blocks, row-major, fully unrolled ----
__device__ __forceinline__ void nd_mm(const double* A, const double* B, double* C) {     // C = A B
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
__device__ __forceinline__ void nd_mtm(const double* A, const double* B, double* C) {    // C = A^T B
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
}

// T1 * T2 of the SE(3) convention include/viekf.h states
__device__ __forceinline__ void nd_compose(const double* T1, const double* T2, double* out) {
  double r[3], q[4];
  q_rota(T1 + 3, T2, r);
  q_otimes(T1 + 3, T2 + 3, q);
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = T1[i] + r[i];
#pragma unroll
  for (int i = 0; i < 4; i++) out[3 + i] = q[i];
}

// acc (6x6, column-major, [pos; att]) += Adj(T)^T C Adj(T) for the symmetric C = [C11 C12; C12^T C22] (3x3 blocks, row-major),
// Adj(T) = [R U; 0 R], R = q.R(), U = [t]x R  (propagate_global_covariance, vi_ekf_kfr.cpp:47-53):
//   [R^T C11 R      R^T X         ]     X = C11 U + C12 R
//   [(R^T X)^T      U^T X + R^T Y ]     Y = C12^T U + C22 R
// The lower-left block is the transpose of the upper-right one bit for bit.
__device__ __forceinline__ void nd_add_adj_cov(const double* T, const double* C11, const double* C12, const double* C22, double* acc) {
  double R[9], S[9], U[9], X[9], Y[9], t0[9], t1[9], C21[9];
  q_R(T + 3, R);
  skew3(T, S);
  nd_mm(S, R, U);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C21[3 * i + j] = C12[3 * j + i];
  nd_mm(C11, U, t0); nd_mm(C12, R, t1);
#pragma unroll
  for (int i = 0; i < 9; i++) X[i] = t0[i] + t1[i];
  nd_mm(C21, U, t0); nd_mm(C22, R, t1);
#pragma unroll
  for (int i = 0; i < 9; i++) Y[i] = t0[i] + t1[i];
  double O11[9], O12[9], O22[9];
  nd_mm(C11, R, t0); nd_mtm(R, t0, O11);
  nd_mtm(R, X, O12);
  nd_mtm(U, X, t0); nd_mtm(R, Y, t1);
#pragma unroll
  for (int i = 0; i < 9; i++) O22[i] = t0[i] + t1[i];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      acc[i + 6 * j] += O11[3 * i + j];
      acc[i + 6 * (3 + j)] += O12[3 * i + j];
      acc[(3 + j) + 6 * i] += O12[3 * i + j];
      acc[(3 + i) + 6 * (3 + j)] += O22[3 * i + j];
    }
}

// get_global_pose (:14-21) and get_global_cov (:23-35) of filter b into pose [7] / cov [36], each where wanted (the flags are
// uniform over the launch; the arrays are the caller's registers either way)
__device__ __forceinline__ void nd_global(const StreamArgs& a, const NodeTabs& t, const NodeOffs& of, int b, bool want_pose, bool want_cov,
                                          double (&pose)[7], double (&cov)[36]) {
  const double* xs = a.x + a.si(b) * a.nxs;
  const double* P = a.P + a.si(b) * a.n * a.ld;
  double p[21];
  if (want_cov) {   // (all 21 in flight before anything else waits)
#pragma unroll
    for (int k = 0; k < 21; k++) p[k] = P[of.o[k]];
  }
  double T[7];
#pragma unroll
  for (int i = 0; i < 7; i++) T[i] = t.node[(long)b * 7 + i];
  if (want_pose) {
    const double rel[7] = {xs[xPOS], xs[xPOS + 1], xs[xPOS + 2], xs[xATT], xs[xATT + 1], xs[xATT + 2], xs[xATT + 3]};
    nd_compose(T, rel, pose);
  }
  if (want_cov) {
#pragma unroll
    for (int i = 0; i < 36; i++) cov[i] = t.cov[(long)b * 36 + i];
    double C11[9], C12[9], C22[9];   // Cx(i, j) = p[i (i + 1) / 2 + j] for i >= j
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const int hi = i > j ? i : j, lo = i > j ? j : i;
        C11[3 * i + j] = p[hi * (hi + 1) / 2 + lo];
        C22[3 * i + j] = p[(3 + hi) * (4 + hi) / 2 + 3 + lo];
        C12[3 * i + j] = p[(3 + j) * (4 + j) / 2 + i];   // Cx(i, 3 + j) = Cx(3 + j, i)
      }
    nd_add_adj_cov(T, C11, C12, C22, cov);
  }
}

// ---- kernels ----
__global__ __launch_bounds__(64) void k_node_reset(int B, NodeTabs t) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
#pragma unroll
  for (int i = 0; i < 7; i++) { const double v = i == 3 ? 1.0 : 0.0; t.node[(long)b * 7 + i] = v; t.tnode[(long)b * 7 + i] = v; }
#pragma unroll
  for (int i = 0; i < 36; i++) t.cov[(long)b * 36 + i] = 0.0;
  t.count[b] = 0;
}

// the end of keyframe_reset (:147-150) for the filters with did_reset[b] != 0.  x_true [B][ldx] or NULL.
__global__ __launch_bounds__(64) void k_node_update(int B, NodeTabs t, const unsigned char* __restrict__ did_reset,
                                                    const double* __restrict__ edges, const double* __restrict__ x_true, int ldx) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  if (!did_reset[b]) return;
  double e[17], T[7], cov[36];
#pragma unroll
  for (int i = 0; i < 17; i++) e[i] = edges[(long)b * 17 + i];
#pragma unroll
  for (int i = 0; i < 7; i++) T[i] = t.node[(long)b * 7 + i];
#pragma unroll
  for (int i = 0; i < 36; i++) cov[i] = t.cov[(long)b * 36 + i];
  double C11[9], C12[9], C22[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) { C11[3 * i + j] = e[7 + i + 3 * j]; C12[3 * i + j] = 0.0; C22[3 * i + j] = 0.0; }
  C22[8] = e[16];
  nd_add_adj_cov(T, C11, C12, C22, cov);   // with the node before it moves (:149)
#pragma unroll
  for (int i = 0; i < 36; i++) t.cov[(long)b * 36 + i] = cov[i];
  const int cnt = t.count[b];
  if (t.cap > 0) {
    const long at = (long)b * t.cap + (cnt % t.cap + t.cap) % t.cap;
#pragma unroll
    for (int i = 0; i < 7; i++) t.tr_node[at * 7 + i] = T[i];
#pragma unroll
    for (int i = 0; i < 17; i++) t.tr_edge[at * 17 + i] = e[i];
  }
  double Tn[7];
  nd_compose(T, e, Tn);                     // :150
#pragma unroll
  for (int i = 0; i < 7; i++) t.node[(long)b * 7 + i] = Tn[i];
  t.count[b] = cnt + 1;
  if (x_true) {   // the reset's map of the estimate (:120-125) applied to the truth
    const double* xt = x_true + (long)b * ldx;
    double q[4];
    q_from_yaw_dev(q_yaw_dev(xt + xATT), q);
#pragma unroll
    for (int i = 0; i < 3; i++) t.tnode[(long)b * 7 + i] = xt[xPOS + i];
#pragma unroll
    for (int i = 0; i < 4; i++) t.tnode[(long)b * 7 + 3 + i] = q[i];
  }
}

__global__ __launch_bounds__(64) void k_node_global(StreamArgs a, NodeTabs t, NodeOffs of, double* __restrict__ pose_out,
                                                    double* __restrict__ cov_out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  double pose[7], cov[36];
  nd_global(a, t, of, b, pose_out != nullptr, cov_out != nullptr, pose, cov);
  if (pose_out) {
#pragma unroll
    for (int i = 0; i < 7; i++) pose_out[(long)b * 7 + i] = pose[i];
  }
  if (cov_out) {
#pragma unroll
    for (int i = 0; i < 36; i++) cov_out[(long)b * 36 + i] = cov[i];
  }
}

// err = [x_true[POS] - pose.t ; x_true[ATT] [-] pose.q], nees = err^T cov^-1 err by a 6x6 Cholesky factorisation in registers;
// info by the rule of k_diag_consistency: j + 1 of the first pivot that is not > 0, and NaN from there
__global__ __launch_bounds__(64) void k_node_global_error(StreamArgs a, NodeTabs t, NodeOffs of, const double* __restrict__ x_true, int ldx,
                                                          double* __restrict__ err_out, double* __restrict__ nees_out,
                                                          int* __restrict__ info_out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.B) return;
  double pose[7], A[36];
  nd_global(a, t, of, b, true, true, pose, A);
  const double* xt = x_true + (long)b * ldx;
  double y[6], d3[3];
#pragma unroll
  for (int i = 0; i < 3; i++) y[i] = xt[xPOS + i] - pose[i];
  q_boxminus_dev(xt + xATT, pose + 3, d3);
#pragma unroll
  for (int i = 0; i < 3; i++) y[3 + i] = d3[i];
  if (err_out) {
#pragma unroll
    for (int i = 0; i < 6; i++) err_out[(long)b * 6 + i] = y[i];
  }
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  int info = 0;
  double nees = 0.0;
#pragma unroll
  for (int j = 0; j < 6; j++) {   // right-looking on the lower triangle, the error as one more row
    const double d = A[j + 6 * j];
    const bool ok = d > 0.0;
    if (!ok && info == 0) info = j + 1;
    const double s = ok ? sqrt(d) : nan, inv = 1.0 / s;
#pragma unroll
    for (int i = j + 1; i < 6; i++) A[i + 6 * j] *= inv;
    y[j] *= inv;
#pragma unroll
    for (int c = j + 1; c < 6; c++) {
#pragma unroll
      for (int i = c; i < 6; i++) A[i + 6 * c] = fma(-A[i + 6 * j], A[c + 6 * j], A[i + 6 * c]);
      y[c] = fma(-y[j], A[c + 6 * j], y[c]);
    }
    nees += y[j] * y[j];
  }
  if (nees_out) nees_out[b] = info ? nan : nees;
  if (info_out) info_out[b] = info;
}

// x_rel = the truth in the true node's frame; one wave64 per filter.  x_rel may be x_true.
__global__ __launch_bounds__(64) void k_node_relative_truth(int B, NodeTabs t, const double* x_true, double* x_rel, int ldx) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const double* xt = x_true + (long)b * ldx;
  double* xr = x_rel + (long)b * ldx;
  for (int c = lane; c < ldx; c += 64)
    if (!(c < xPOS + 3) && !(c >= xATT && c < xATT + 4)) xr[c] = xt[c];
  if (lane == 0) {
    double T[7];
#pragma unroll
    for (int i = 0; i < 7; i++) T[i] = t.tnode[(long)b * 7 + i];
    const double d[3] = {xt[xPOS] - T[0], xt[xPOS + 1] - T[1], xt[xPOS + 2] - T[2]};
    const double qi[4] = {T[3], -T[4], -T[5], -T[6]}, qt[4] = {xt[xATT], xt[xATT + 1], xt[xATT + 2], xt[xATT + 3]};
    double p[3], q[4];
    q_rotp(T + 3, d, p);
    q_otimes(qi, qt, q);
#pragma unroll
    for (int i = 0; i < 3; i++) xr[xPOS + i] = p[i];
#pragma unroll
    for (int i = 0; i < 4; i++) xr[xATT + i] = q[i];
  }
}

}  // namespace viekf
