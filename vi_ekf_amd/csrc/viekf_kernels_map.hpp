// viekf_kernels_map.hpp -- the device-resident landmark map (include/viekf_map.h): every feature slot of every
// filter as a 3-D position with a 3x3 covariance, in the node frame and in the global frame; a store of them keyed by the
// frame intake's feature ids; and the metric error against the landmark a feature was drawn from.
//
//   k_map_landmarks  the live query: l, Sigma = J P9 J^T, l_G, Sigma_G of every slot
//   k_map_update     the same l_G / Sigma_G of the valid tracked slots into the store, entry id % capacity; which of several
//                    ids of one residue is written is decided by comparing the filter's ids in LDS, not by store order
//   k_map_error      l against the true landmark in the true node's frame, its NEES through a 3x3 Cholesky factorisation in
//                    registers, l_G against the true landmark
// Lane -> work: ONE WORKGROUP PER FILTER, A LANE PER FEATURE SLOT (a loop when num_features exceeds the block), not a lane per
// filter as in viekf_kernels_node.hpp.  In column-major P the 18 feature-by-body elements of neighbouring slots lie 24 bytes
// apart within a column, so a wave's loads touch few lines; the 17 body state values, the 21 body elements of P and the nodes
// are the same for every slot and are read once per workgroup into LDS (mp_shared); only the 6 elements of a slot's diagonal
// block are scattered.  All loads of a lane are issued before the first use.  fp64 throughout, the small matrices fully
// unrolled in registers, no scratch.  READ-ONLY on the batch; only the lower triangle of P is read.
#pragma once
#include "viekf_kernels_node.hpp"

namespace viekf {

// the store, [B][cap] entries
struct MapTabs {
  int* id;          // [B][cap]     the intake's feature id, -1: empty
  double* pos;      // [B][cap][3]  l_G
  double* cov;      // [B][cap][6]  Sigma_G: xx, yx, yy, zx, zy, zz
  int* nobs;        // [B][cap]
  int* ncount;      // [B][cap]     the node graph's reset count at the write
  int cap;
};

// what the slots of one filter share, in LDS: the body state, the lower triangle of P on {POS, ATT} x {POS, ATT} in the order
// k = i (i + 1) / 2 + j of viekf_kernels_node.hpp, the node and the true node
constexpr int MP_X = 0, MP_P = 17, MP_NODE = 38, MP_TNODE = 45, MP_SH = 52;
constexpr int MP_MAX_T = 256;   // threads of a workgroup: 64, 128 or 256 by num_features (map_block, viekf_capi_map.hpp)

// Threads 0 .. 51 of the workgroup (>= 64 threads) read the shared values of filter b once.  node / tnode [B][7] or NULL (the
// identity).  Ends with a barrier.
__device__ __forceinline__ void mp_shared(const StreamArgs& a, const double* __restrict__ node, const double* __restrict__ tnode, int b,
                                          double* sh) {
  const int t = threadIdx.x;
  const double* xs = a.x + a.si(b) * a.nxs;
  const double* P = a.P + a.si(b) * a.n * a.ld;
  if (t < MP_P) {
    sh[MP_X + t] = xs[t];
  } else if (t < MP_NODE) {
    const int k = t - MP_P;
    int i = 0;
    while ((i + 1) * (i + 2) / 2 <= k) i++;
    const int j = k - i * (i + 1) / 2;
    const int ri = i < 3 ? dxPOS + i : dxATT + i - 3, rj = j < 3 ? dxPOS + j : dxATT + j - 3;
    sh[t] = P[ri + (long)rj * a.ld];
  } else if (t < MP_SH) {
    const int k = t < MP_TNODE ? t - MP_NODE : t - MP_TNODE;
    const double* src = t < MP_TNODE ? node : tnode;
    sh[t] = src ? src[(long)b * 7 + k] : (k == 3 ? 1.0 : 0.0);
  }
  __syncthreads();
}

// Slot j (0 <= j < N: every address is inside the filter's x and P, whatever len_features is) of filter b: l [3] and Sigma [6]
// in the node frame.  Returns whether the slot is valid (j < len, rho finite and > 0); the outputs of an invalid slot are
// whatever the arithmetic gives and are replaced by the caller.
__device__ __forceinline__ bool mp_landmark(const StreamArgs& a, const double* sh, int b, int j, int len, double (&l)[3], double (&S)[6]) {
  const double* xs = a.x + a.si(b) * a.nxs;
  const double* P = a.P + a.si(b) * a.n * a.ld;
  const DevParams& dp = a.prm(b);
  const int r = dxZ + 3 * j;
  const long ld = a.ld;
  double pf[18], pd[6], xf[5];
  // every load of this lane, before anything waits: 18 feature-by-body elements (neighbouring lanes 24 bytes apart within a
  // column), the 6 of the diagonal block, the feature state
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int c = 0; c < 6; c++) pf[6 * k + c] = P[(r + k) + (c < 3 ? dxPOS + c : dxATT + c - 3) * ld];
#pragma unroll
  for (int k = 0; k < 3; k++)
#pragma unroll
    for (int m = 0; m <= k; m++) pd[k * (k + 1) / 2 + m] = P[(r + k) + (r + m) * ld];
#pragma unroll
  for (int i = 0; i < 5; i++) xf[i] = xs[xZ + 5 * j + i];
  // P9(i, k) on {POS, ATT, feature j}, from the lower triangle (indices are constants after unrolling)
  auto p9 = [&](int i, int k) -> double {
    const int hi = i > k ? i : k, lo = i > k ? k : i;
    if (hi < 6) return sh[MP_P + hi * (hi + 1) / 2 + lo];
    if (lo < 6) return pf[6 * (hi - 6) + lo];
    return pd[(hi - 6) * (hi - 5) / 2 + (lo - 6)];
  };
  const double rho = xf[4];
  const bool ok = j < len && rho > 0.0 && __builtin_isfinite(rho);
  const double inv = 1.0 / rho;
  double t1[3], t2[3], zeta[3], pc[3], rc[3], bv[3], rb[3];
  bearing_frame(xf, t1, t2, zeta);          // T_zeta = [t1 t2], zeta = rota(q_zeta, e_z)
#pragma unroll
  for (int i = 0; i < 3; i++) pc[i] = zeta[i] * inv;
  q_rota(dp.q_b_c, pc, rc);
#pragma unroll
  for (int i = 0; i < 3; i++) bv[i] = dp.p_b_c[i] + rc[i];
  q_rota(sh + MP_X + xATT, bv, rb);
#pragma unroll
  for (int i = 0; i < 3; i++) l[i] = sh[MP_X + xPOS + i] + rb[i];
  // J = [I | G], G = [-Ra^T [b]x | -Ra^T Rc^T [zeta]x T_zeta / rho | -Ra^T Rc^T zeta / rho^2] row-major 3 x 6: with P9 split into
  // the position block a and the rest r, Sigma = P_aa + G P_ra + (G P_ra)^T + G P_rr G^T (the identity block is not multiplied)
  double Ra[9], Rc[9], Sb[9], M[9], zt1[3], zt2[3], G[18];
  q_R(sh + MP_X + xATT, Ra);
  q_R(dp.q_b_c, Rc);
  skew3(bv, Sb);
  cross3(zeta, t1, zt1);                    // the columns of [zeta]x T_zeta
  cross3(zeta, t2, zt2);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) M[3 * i + k] = Ra[i] * Rc[3 * k] + Ra[3 + i] * Rc[3 * k + 1] + Ra[6 + i] * Rc[3 * k + 2];   // Ra^T Rc^T
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int k = 0; k < 3; k++) G[6 * i + k] = -(Ra[i] * Sb[k] + Ra[3 + i] * Sb[3 + k] + Ra[6 + i] * Sb[6 + k]);
    G[6 * i + 3] = -(M[3 * i] * zt1[0] + M[3 * i + 1] * zt1[1] + M[3 * i + 2] * zt1[2]) * inv;
    G[6 * i + 4] = -(M[3 * i] * zt2[0] + M[3 * i + 1] * zt2[1] + M[3 * i + 2] * zt2[2]) * inv;
    G[6 * i + 5] = -(M[3 * i] * zeta[0] + M[3 * i + 1] * zeta[1] + M[3 * i + 2] * zeta[2]) * inv * inv;
  }
  double U[9], W[18];                       // G P_ra (3 x 3), G P_rr (3 x 6)
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += G[6 * i + k] * p9(3 + k, c);
      U[3 * i + c] = s;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) s += G[6 * i + k] * p9(3 + k, 3 + c);
      W[6 * i + c] = s;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k <= i; k++) {
      double s = p9(i, k) + U[3 * i + k] + U[3 * k + i];
#pragma unroll
      for (int c = 0; c < 6; c++) s += W[6 * i + c] * G[6 * k + c];
      S[i * (i + 1) / 2 + k] = s;
    }
  return ok;
}

// l_G = T.t + rota(T.q, l), Sigma_G = R(T.q)^T Sigma R(T.q) for the node T [7] (in LDS)
__device__ __forceinline__ void mp_global(const double* T, const double (&l)[3], const double (&S)[6], double (&lg)[3], double (&Sg)[6]) {
  double R[9], r[3], F[9], X[9];
  q_R(T + 3, R);
  q_rota(T + 3, l, r);
#pragma unroll
  for (int i = 0; i < 3; i++) lg[i] = T[i] + r[i];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) F[3 * i + k] = S[i > k ? i * (i + 1) / 2 + k : k * (k + 1) / 2 + i];
  nd_mm(F, R, X);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k <= i; k++) Sg[i * (i + 1) / 2 + k] = R[i] * X[k] + R[3 + i] * X[3 + k] + R[6 + i] * X[6 + k];
}

__device__ __forceinline__ int mp_len(const StreamArgs& a, int b) { return min(max(a.len[b], 0), a.N); }

// ---- kernels: grid = B workgroups of 64, 128 or 256 threads ----
__global__ __launch_bounds__(MP_MAX_T) void k_map_landmarks(StreamArgs a, const double* __restrict__ node, double* __restrict__ pos_n,
                                                            double* __restrict__ cov_n, double* __restrict__ pos_g,
                                                            double* __restrict__ cov_g) {
  __shared__ double sh[MP_SH];
  const int b = blockIdx.x;
  if (b >= a.B) return;
  mp_shared(a, node, nullptr, b, sh);
  const int len = mp_len(a, b);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int j = threadIdx.x; j < a.N; j += blockDim.x) {
    double l[3], S[6], lg[3], Sg[6];
    const bool ok = mp_landmark(a, sh, b, j, len, l, S);
    mp_global(sh + MP_NODE, l, S, lg, Sg);
    const long e = (long)b * a.N + j;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      if (pos_n) pos_n[e * 3 + i] = ok ? l[i] : nan;
      if (pos_g) pos_g[e * 3 + i] = ok ? lg[i] : nan;
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
      if (cov_n) cov_n[e * 6 + i] = ok ? S[i] : nan;
      if (cov_g) cov_g[e * 6 + i] = ok ? Sg[i] : nan;
    }
  }
}

// tab [B][N], tlen [B]: the intake's id table; count [B] the node graph's reset counts or NULL.  Dynamic LDS: N ints.
__global__ __launch_bounds__(MP_MAX_T) void k_map_update(StreamArgs a, const int* __restrict__ tab, const int* __restrict__ tlen,
                                                         const double* __restrict__ node, const int* __restrict__ count, MapTabs m) {
  __shared__ double sh[MP_SH];
  extern __shared__ __attribute__((aligned(16))) int mp_ids[];
  const int b = blockIdx.x;
  if (b >= a.B) return;
  const int len = mp_len(a, b);
  if (len != min(max(tlen[b], 0), a.N)) return;   // a stale table: the store keeps every bit (the same in every thread)
  mp_shared(a, node, nullptr, b, sh);
  const double* xs = a.x + a.si(b) * a.nxs;
  // the ids that want an entry: the valid tracked slots
  for (int j = threadIdx.x; j < a.N; j += blockDim.x) {
    const double rho = xs[xZ + 5 * j + 4];
    const int g = tab[(long)b * a.N + j];
    mp_ids[j] = (j < len && rho > 0.0 && __builtin_isfinite(rho)) ? g : -1;
  }
  __syncthreads();
  const int cnt = count ? count[b] : 0;
  for (int j = threadIdx.x; j < a.N; j += blockDim.x) {
    const int g = mp_ids[j];
    const int e = g >= 0 ? g % m.cap : -1;
    bool win = g >= 0;
    for (int i = 0; i < len; i++) {   // (every lane reads the same word: a broadcast)
      const int o = mp_ids[i];
      if (o >= 0 && o % m.cap == e && (o > g || (o == g && i > j))) win = false;   // the larger id; of equal ids the later slot
    }
    double l[3], S[6], lg[3], Sg[6];
    (void)mp_landmark(a, sh, b, j, len, l, S);
    mp_global(sh + MP_NODE, l, S, lg, Sg);
    if (win) {
      const long at = (long)b * m.cap + e;
      const int seen = m.id[at] == g ? m.nobs[at] + 1 : 1;
      m.id[at] = g;
#pragma unroll
      for (int i = 0; i < 3; i++) m.pos[at * 3 + i] = lg[i];
#pragma unroll
      for (int i = 0; i < 6; i++) m.cov[at * 6 + i] = Sg[i];
      m.nobs[at] = seen;
      m.ncount[at] = cnt;
    }
  }
}

// lm_true [lm_per ? B : 1][L][3]; frame_ids, landmark [B][M].  Dynamic LDS: 2 M ints.
__global__ __launch_bounds__(MP_MAX_T) void k_map_error(StreamArgs a, const int* __restrict__ tab, const int* __restrict__ tlen,
                                                        const double* __restrict__ node, const double* __restrict__ tnode,
                                                        const double* __restrict__ lm_true, int lm_per, int L,
                                                        const int* __restrict__ frame_ids, const int* __restrict__ landmark, int M,
                                                        double* __restrict__ err_n, double* __restrict__ nees_out,
                                                        int* __restrict__ info_out, double* __restrict__ err_g) {
  __shared__ double sh[MP_SH];
  extern __shared__ __attribute__((aligned(16))) int mp_ids[];
  const int b = blockIdx.x;
  if (b >= a.B) return;
  int* fid = mp_ids;
  int* flm = mp_ids + M;
  for (int i = threadIdx.x; i < M; i += blockDim.x) { fid[i] = frame_ids[(long)b * M + i]; flm[i] = landmark[(long)b * M + i]; }
  mp_shared(a, node, tnode, b, sh);   // (its barrier covers the frame's rows as well)
  const int len = mp_len(a, b);
  const bool stale = len != min(max(tlen[b], 0), a.N);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  for (int j = threadIdx.x; j < a.N; j += blockDim.x) {
    double l[3], S[6], lg[3], Sg[6];
    bool ok = mp_landmark(a, sh, b, j, len, l, S) && !stale;
    mp_global(sh + MP_NODE, l, S, lg, Sg);
    const int g = tab[(long)b * a.N + j];
    int k = -1;
    if (ok && g >= 0) {
      for (int i = M - 1; i >= 0; i--)   // (the FIRST match, as viekf_sim_truth_state)
        if (fid[i] == g) k = flm[i];
    }
    ok = ok && k >= 0 && k < L;
    const double* lt = lm_true + (lm_per ? (long)b * L * 3 : 0L) + 3L * (ok ? k : 0);
    double d[3] = {0.0, 0.0, 0.0}, y[3], eg[3] = {0.0, 0.0, 0.0};
    if (ok) {
#pragma unroll
      for (int i = 0; i < 3; i++) { d[i] = lt[i] - sh[MP_TNODE + i]; eg[i] = lt[i] - lg[i]; }
    }
    q_rotp(sh + MP_TNODE + 3, d, y);
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] -= l[i];
    const long e = (long)b * a.N + j;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      if (err_n) err_n[e * 3 + i] = ok ? y[i] : nan;
      if (err_g) err_g[e * 3 + i] = ok ? eg[i] : nan;
    }
    // right-looking Cholesky on the lower triangle, the error as one more row (as k_node_global_error)
    int info = 0;
    double nees = 0.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double dg = S[c * (c + 1) / 2 + c];
      const bool pos = dg > 0.0;
      if (!pos && info == 0) info = c + 1;
      const double s = pos ? sqrt(dg) : nan, iv = 1.0 / s;
#pragma unroll
      for (int i = c + 1; i < 3; i++) S[i * (i + 1) / 2 + c] *= iv;
      y[c] *= iv;
#pragma unroll
      for (int q = c + 1; q < 3; q++) {
#pragma unroll
        for (int i = q; i < 3; i++) S[i * (i + 1) / 2 + q] = fma(-S[i * (i + 1) / 2 + c], S[q * (q + 1) / 2 + c], S[i * (i + 1) / 2 + q]);
        y[q] = fma(-y[c], S[q * (q + 1) / 2 + c], y[q]);
      }
      nees += y[c] * y[c];
    }
    if (nees_out) nees_out[e] = (ok && !info) ? nees : nan;
    if (info_out) info_out[e] = ok ? info : 0;
  }
}

}  // namespace viekf
