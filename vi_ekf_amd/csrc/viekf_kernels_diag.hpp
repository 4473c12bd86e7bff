// viekf_kernels_diag.hpp -- consistency diagnostics (include/viekf_diag.h): per filter one Cholesky
// factorisation of the active block of P, read from the LOWER triangle only, and what follows from it -- log det P, the
// whitened error y = L^-1 (x_true [-] x) and the NEES of the leading blocks -- plus the innovation statistics of the
// reference's measurement models at the current state.  Read-only: nothing here writes x, P, len or the flags.
//
// k_diag_consistency, one workgroup per filter, __syncthreads() only:
//   storage   the lower triangle PACKED by columns with the error e as one more row: column j holds rows j .. m (row m = e),
//             element (i, j) at cs(j) + i - j, cs(j) = j (m + 1) - j (j - 1) / 2.  In LDS where that fits (LDS = true), in a
//             device workspace otherwise -- the same code either way.  Threads that walk down a column touch consecutive
//             doubles: conflict-free in LDS, coalesced in the workspace.
//   e row     Forward substitution IS the factorisation of one more row: with e stored as row m, the panel solve and the
//             trailing update that turn A into L turn e into y = L^-1 e, so there is no substitution phase.
//   panel     right-looking, 16 columns a step, three barriers a step.  Every wave factors the 16 x 16 diagonal block itself:
//             lanes 0..15 hold one row each in registers and the pivots / multipliers travel by v_readlane (no LDS, no
//             barrier); lanes 16..63 of the same wave hold 48 rows below the block and take the same multipliers, which is
//             their triangular solve.  Wave 0 stores the block.
//   trailing  rank-16 update of what lies below and right of the panel: per thread a 4 x 4 register tile whose rows and
//             columns are 16 and T/16 apart, so that the lanes of a wave read 16 consecutive doubles of a panel column
//             (the others broadcast): 8 LDS reads per 16 FMAs.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"

namespace viekf {

constexpr int DG_NB = 16;    // panel width
constexpr int DG_T = 512;    // threads per workgroup: 8 waves x 48 rows below a panel in one pass up to n = 399

// doubles of the packed storage of an n x n lower triangle and the error row
__host__ __device__ inline long diag_packed_doubles(int n) { return (long)n * (n + 1) / 2 + n; }

__device__ __forceinline__ double dg_bcast(double v, int lane) {   // lane: uniform (a constant after unrolling)
  const long long u = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffLL), lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(u >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// A (packed, R = m + 1 rows) -> L in place, row m -> L^-1 row m.  Returns 0 or j + 1 of the first pivot that is not > 0
// (the same in every thread).  Ends with a barrier.
template <int T>
__device__ __forceinline__ int dg_factor(double* __restrict__ A, const int m) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = T / 64, TCN = T / 16;
  const int R = m + 1;
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  auto cs = [&](int j) { return (long)j * R - (long)j * (j - 1) / 2; };
  int info = 0;
  for (int k0 = 0; k0 < m; k0 += DG_NB) {
    const int nb = min(DG_NB, m - k0);
    const int r0 = k0 + nb;        // first row below the panel
    const int nrows = R - r0;      // rows below it (the error row included)
    double a[DG_NB];
    for (int q = 0; q == 0 || q * NW * 48 < nrows; q++) {
      const bool fresh = q == 0;
      const int idx = (q * NW + wave) * 48 + lane - 16;
      const int i = lane < 16 ? k0 + lane : r0 + idx;
      const bool valid = lane < 16 ? i < m : idx < nrows;
      if (fresh || lane >= 16) {   // (on a later pass lanes 0..15 keep the factored block)
#pragma unroll
        for (int c = 0; c < DG_NB; c++) {
          double v = 0.0;
          if (lane < 16) {
            if (valid && c <= lane) v = A[cs(k0 + c) + (i - k0 - c)];
            else if (!valid && c == lane) v = 1.0;   // (a row past m: identity, a pivot of 1)
          } else if (valid && c < nb) v = A[cs(k0 + c) + (i - k0 - c)];
          a[c] = v;
        }
      }
      if (fresh) __syncthreads();   // every wave holds the block before wave 0 overwrites it
#pragma unroll
      for (int j = 0; j < DG_NB; j++) {
        const double d = dg_bcast(a[j], j);
        double s = d;
        if (fresh) {
          const bool ok = d > 0.0;
          if (!ok && info == 0) info = k0 + j + 1;
          s = ok ? sqrt(d) : nan;
        }
        const double inv = 1.0 / s;
        const bool upd = fresh || lane >= 16;
        const double aj = upd ? (lane == j ? s : a[j] * inv) : a[j];
        a[j] = aj;
#pragma unroll
        for (int p = j + 1; p < DG_NB; p++) {
          const double lpj = dg_bcast(aj, p);
          a[p] = upd ? fma(-aj, lpj, a[p]) : a[p];
        }
      }
      if (lane >= 16 || (fresh && wave == 0)) {
#pragma unroll
        for (int c = 0; c < DG_NB; c++)
          if (valid && c < nb && (lane >= 16 || c <= lane)) A[cs(k0 + c) + (i - k0 - c)] = a[c];
      }
    }
    __syncthreads();
    // trailing update: A(i, j) -= sum_c L(i, k0 + c) L(j, k0 + c) for r0 <= j < m, j <= i < R
    const int ncols = m - r0;
    const int tr = tid & 15, tc = tid >> 4;
    for (int cb = 0; cb < ncols; cb += 4 * TCN)
      for (int rb = (cb >> 6) << 6; rb < nrows; rb += 64) {
        const int li0 = rb + tr, lj0 = cb + tc;
        if (li0 + 48 < lj0 || lj0 >= ncols || li0 >= nrows) continue;   // (nothing of this thread's tile on or below the diagonal)
        double acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
          for (int w = 0; w < 4; w++) acc[u][w] = 0.0;
        for (int c = 0; c < nb; c++) {
          const double* col = A + (cs(k0 + c) - (k0 + c) + r0);   // col[l] = L(r0 + l, k0 + c)
          double rv[4], cv[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int li = li0 + 16 * u, lj = lj0 + TCN * u;
            rv[u] = li < nrows ? col[li] : 0.0;
            cv[u] = lj < ncols ? col[lj] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 4; u++)
#pragma unroll
            for (int w = 0; w < 4; w++) acc[u][w] = fma(rv[u], cv[w], acc[u][w]);
        }
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const int lj = lj0 + TCN * w;
          if (lj >= ncols) continue;
          double* dst = A + (cs(r0 + lj) - lj);   // dst[l] = A(r0 + l, r0 + lj)
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int li = li0 + 16 * u;
            if (li < nrows && li >= lj) dst[li] -= acc[u][w];
          }
        }
      }
    __syncthreads();
  }
  return info;
}

// Filters b0 + blockIdx.x.  LDS: the packed triangle lives in dynamic LDS (diag_packed_doubles(n) doubles); otherwise in
// ws + blockIdx.x * ws_stride.  x_true [B][nx] or NULL (then e = 0); every output may be NULL.
template <int T, bool LDS>
__global__ __launch_bounds__(T) void k_diag_consistency(StreamArgs a, int b0, const double* __restrict__ x_true, double* __restrict__ ws,
                                                        long ws_stride, double* __restrict__ logdet, double* __restrict__ nees,
                                                        double* __restrict__ whitened, int* __restrict__ info_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = b0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (b >= a.B) return;
  constexpr int NW = T / 64;
  const int len = min(max(a.len[b], 0), a.N);
  const int m = dxZ + 3 * len, R = m + 1, ld = a.ld;
  double* A;
  if constexpr (LDS) A = smem;
  else A = ws + (long)blockIdx.x * ws_stride;
  const double* P = a.P + a.si(b) * a.n * ld;
  const double* x2 = a.x + a.si(b) * a.nxs;
  auto cs = [&](int j) { return (long)j * R - (long)j * (j - 1) / 2; };
  // the lower triangle, once: a wave reads 64 consecutive rows of a column (the column stride is ld), 8 columns in flight
  for (int ib = 0; ib < m; ib += 64) {
    const int i = ib + lane, jmax = min(m, ib + 64);
    for (int j0 = wave; j0 < jmax; j0 += 8 * NW) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int j = j0 + u * NW;
        v[u] = (j < jmax && j <= i && i < m) ? P[i + (long)j * ld] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int j = j0 + u * NW;
        if (j < jmax && j <= i && i < m) A[cs(j) + (i - j)] = v[u];
      }
    }
  }
  // e = x_true [-] x as row m (vi_ekf_helper.cpp:100-111, as k_boxops)
  if (x_true) {
    const double* x1 = x_true + (long)b * a.nx;
    if (tid == 0) {
      double o[16];
      body_boxminus_dev(x1, x2, o);
      for (int j = 0; j < 16; j++) A[cs(j) + (m - j)] = o[j];
    }
    for (int f = tid - 64; f < len; f += T)
      if (f >= 0) {
        double d[3];
        feat_boxminus_dev(x1 + xZ + 5 * f, x2 + xZ + 5 * f, d);
        const int j = dxZ + 3 * f;
        for (int k = 0; k < 3; k++) A[cs(j + k) + (m - j - k)] = d[k];
      }
  } else {
    for (int j = tid; j < m; j += T) A[cs(j) + (m - j)] = 0.0;
  }
  __syncthreads();
  const int info = dg_factor<T>(A, m);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  if (whitened)
    for (int j = tid; j < a.n; j += T) whitened[(long)b * a.n + j] = j < m ? A[cs(j) + (m - j)] : 0.0;
  if (wave == 0) {   // lane-strided sums in a fixed order, then a butterfly: the same bits on every run
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int j = lane; j < m; j += 64) {
      const double y = A[cs(j) + (m - j)], y2 = y * y;
      if (j < 3) s[0] += y2;
      if (j < 9) s[1] += y2;
      if (j < 16) s[2] += y2;
      s[3] += y2;
      s[4] += log(A[cs(j)]);
    }
#pragma unroll
    for (int k = 0; k < 5; k++)
      for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off);
    if (lane == 0) {
      if (logdet) logdet[b] = info ? nan : 2.0 * s[4];
      if (nees)
        for (int k = 0; k < 4; k++) nees[(long)b * 4 + k] = s[k];
      if (info_out) info_out[b] = info;
    }
  }
}

// One thread per (filter, measurement): residual, S = H P H^T + R and nis = r^T S^-1 r of measurement model `type` at the
// current state, in the arithmetic of k_update_generic's gate (vi_ekf_meas.cpp:205-235).  H has at most six non-zero
// columns (meas_model), so H P H^T is a sum over at most 6 x 6 entries of P, each read from the lower triangle.
__global__ __launch_bounds__(64) void k_diag_innovation(StreamArgs a, int type, int M, const double* __restrict__ z_all, int zdim,
                                                        const int* __restrict__ slot_all, const double* __restrict__ R_all, int rdim,
                                                        long rsb, long rsm, double* __restrict__ nis, double* __restrict__ residual,
                                                        double* __restrict__ S_out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)a.B * M) return;
  const int b = (int)(e / M), mi = (int)(e - (long)b * M);
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  const int len = min(max(a.len[b], 0), a.N);
  const bool needs_slot = meas_needs_slot(type);
  const int slot = (needs_slot && slot_all) ? slot_all[e] : 0;
  double r3[3] = {nan, nan, nan}, S[9], mahal = nan;
  for (int i = 0; i < 9; i++) S[i] = nan;
  if (!needs_slot || (slot >= 0 && slot < len)) {
    const double* xs = a.x + a.si(b) * a.nxs;
    const double* P = a.P + a.si(b) * a.n * a.ld;
    const double* z = z_all + e * zdim;
    const double* R = R_all + (long)b * rsb + (long)mi * rsm;   // column-major rdim x rdim
    int cols[6], nc = 0;
    double Hc[18], zhat[4] = {0.0, 0.0, 0.0, 0.0}, W[6][3], Sr[9], Si[9];
    meas_model(type, xs, slot, a.prm(b), zhat, cols, Hc, nc);
    r3[0] = r3[1] = r3[2] = 0.0;
    meas_residual(type, z, zhat, zdim, r3);
    for (int ci = 0; ci < nc; ci++) {                                  // W = P H^T at the rows H touches
      double w[3] = {0.0, 0.0, 0.0};
      for (int c = 0; c < nc; c++) {
        const int hi = max(cols[ci], cols[c]), lo = min(cols[ci], cols[c]);
        const double pv = P[hi + (long)lo * a.ld];
        for (int q = 0; q < rdim; q++) w[q] += pv * Hc[q * 6 + c];
      }
      for (int q = 0; q < 3; q++) W[ci][q] = w[q];
    }
    for (int p = 0; p < rdim; p++)
      for (int q = 0; q < rdim; q++) {
        double s = 0.0;
        for (int c = 0; c < nc; c++) s += Hc[p * 6 + c] * W[c][q];
        Sr[p * rdim + q] = s + R[p + q * rdim];
      }
    small_inverse_dev(rdim, Sr, Si);
    mahal = 0.0;
    for (int q = 0; q < rdim; q++) {
      double t = 0.0;
      for (int p = 0; p < rdim; p++) t += r3[p] * Si[p * rdim + q];
      mahal += t * r3[q];
    }
    for (int i = 0; i < 9; i++) S[i] = 0.0;
    for (int p = 0; p < rdim; p++)
      for (int q = 0; q < rdim; q++) S[p + q * rdim] = Sr[p * rdim + q];
    for (int i = rdim; i < 3; i++) r3[i] = 0.0;
  }
  nis[e] = mahal;
  if (residual)
    for (int i = 0; i < 3; i++) residual[e * 3 + i] = r3[i];
  if (S_out)
    for (int i = 0; i < 9; i++) S_out[e * 9 + i] = S[i];
}

}  // namespace viekf
