// viekf_onepass.hpp -- what the kernels that apply a measurement's updates in ONE pass over P share (k_update_body_n,
// k_update_depths, k_update_pixvels): the partial-update factor, fix_depth on the rho diagonals held in
// LDS, gain, correction and downdate of a rank-R entry, the left-looking rebuild, the prologue's loads, the epilogue and the
// trailing pass.  The fused routes are defined as bit for bit the entry-by-entry route: every rounded operation they share is
// stated here, once, so that each place contracts alike.  (The admission of an entry and the state correction behind an
// applied one stay written out in the kernels: as functions they changed the kernels' listings)
// Device functions only, no __global__: any header may include it.
#pragma once
#include "viekf_kernel_args.hpp"

namespace viekf {

// L(i, j) of the partial update (vi_ekf_meas.cpp:254-262), and L where the partial update may be off (1 then).  Which of
// the two a place calls is what keeps its kernel's register numbers: k_update_depths and the trailing pass choose at the call
// site (`partial ? partial_L(li, lj) : 1.0`), the PIXEL_VEL kernels in here, each as before the factor was stated once.
__device__ __forceinline__ double partial_L(double li, double lj) { return lj + li - li * lj; }
__device__ __forceinline__ double partial_L(bool partial, double li, double lj) { return partial ? partial_L(li, lj) : 1.0; }

// fix_depth_one (viekf_kernel_args.hpp) with P(rho, rho) of the filter's features in the array D
__device__ __forceinline__ void fix_depth_diag(double* xs, double* D, int f, const DevParams& p, unsigned& flag) {
  const int xR = xZ + 5 * f + 4;
  double rho = xs[xR];
  fix_depth_rule(rho, 1.0 / (2.0 * p.min_depth), flag, [&](double e2) { D[f] += e2; }, [&] { D[f] = p.P0_feat[2]; });
  xs[xR] = rho;
}

// A rank-R entry on one row of its W = P H^T (w[R]) and its S^-1 (row-major R x R) -- operation by operation what
// k_update_generic does:  a gain element K[q] = sum_p w[p] S^-1[p][q];  an element of the correction, sum_q (l K[q]) r[q];
// the downdate of one element, v - L sum_q K_hi[q] W_lo[q] with hi = max(i, j), lo = min(i, j).
template <int R>
__device__ __forceinline__ double onepass_gain(const double (&w)[R], const double* Si, int q) {
  double k = 0.0;
#pragma unroll
  for (int p = 0; p < R; p++) k += w[p] * Si[p * R + q];
  return k;
}
template <int R>
__device__ __forceinline__ double onepass_dx(double l, const double (&k)[R], const double* r) {
  double s = 0.0;
#pragma unroll
  for (int q = 0; q < R; q++) s += (l * k[q]) * r[q];
  return s;
}
template <int R>
__device__ __forceinline__ double onepass_downdate(double v, double L, const double (&k)[R], const double (&w)[R]) {
  double t = 0.0;
#pragma unroll
  for (int q = 0; q < R; q++) t += k[q] * w[q];
  return v - L * t;
}

// The same on the layout the chains keep: an applied entry's W as [R][nW] (Wk) and its S^-1 (Sk).
template <int R>
__device__ __forceinline__ void onepass_row(const double* Wk, int nW, int i, double (&w)[R]) {
#pragma unroll
  for (int q = 0; q < R; q++) w[q] = Wk[q * nW + i];
}
template <int R>
__device__ __forceinline__ void onepass_gains(const double* Wk, int nW, int i, const double* Sk, double (&k)[R]) {
  double w[R];
  onepass_row<R>(Wk, nW, i, w);
#pragma unroll
  for (int q = 0; q < R; q++) k[q] = onepass_gain<R>(w, Sk, q);
}
template <int R>
__device__ __forceinline__ double onepass_apply(double v, double L, const double* Wk, int nW, const double* Sk, int hi, int lo) {
  double k[R], w[R];
  onepass_gains<R>(Wk, nW, hi, Sk, k);
  onepass_row<R>(Wk, nW, lo, w);
  return onepass_downdate<R>(v, L, k, w);
}

// Left-looking: element (hi, lo) of the current P from its value v in the start P -- minus the downdates of the napp applied
// entries (Wall [entry][R][nW], Sinv [entry][R * R]), in order, UNR of them in flight.  The caller takes a rho diagonal from D.
template <int R, int UNR>
__device__ __forceinline__ double onepass_rebuild(double v, double L, const double* Wall, int nW, const double* Sinv, int napp, int hi,
                                                  int lo) {
#pragma unroll UNR
  for (int k = 0; k < napp; k++) v = onepass_apply<R>(v, L, Wall + (long)k * R * nW, nW, Sinv + R * R * k, hi, lo);
  return v;
}

// The prologue's loads: x, lambda and the rho diagonals.
template <int T>
__device__ __forceinline__ void onepass_load(const StreamArgs& a, int b, const double* xg, const double* P, int len, double* xs, double* lam,
                                             double* D) {
  const int tid = threadIdx.x, ld = a.ld;
  for (int i = tid; i < xZ + 5 * len; i += T) xs[i] = xg[i];
  for (int i = tid; i < a.n; i += T) lam[i] = a.lam(b)[i];
  for (int f = tid; f < len; f += T) { const long dR = dxZ + 3 * f + 2; D[f] = P[dR + dR * ld]; }
}

// The trailing pass for napp applied entries of rank R (Wall [entry][R][nW], Sinv [entry][R * R]): the lower triangle of the
// active block, rho diagonals excepted (they are stored from D).  A lane keeps ROW i (64 consecutive rows per wave: a column's
// segment is 512 contiguous bytes); a wave takes UN adjacent columns at a time, loads before arithmetic; per entry a lane
// reads its own W (conflict-free) and forms its gains, S^-1 and the UN columns' W are broadcasts.  The entries run innermost,
// in order, on the values held in registers.
template <int T, int R>
__device__ __forceinline__ void onepass_trailing(double* __restrict__ P, int ld, int nact, int nW, int napp, bool partial,
                                                 const double* Wall, const double* Sinv, const double* lam) {
  constexpr int NW = T / 64;   // waves
  constexpr int UN = 8;        // columns a wave has in flight
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r0 = 0; r0 < nact; r0 += 64) {
    const int i = r0 + lane;
    const bool valid = i < nact;
    const int ir = valid ? i : 0;
    const double li = lam[ir];
    const bool isrho = i >= dxZ && (i - dxZ) % 3 == 2;
    const int jend = min(r0 + 63, nact - 1);
    for (int j0 = wid * UN; j0 <= jend; j0 += NW * UN) {
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
      for (int u = 0; u < UN; u++) {
        const double lj = lam[min(j0 + u, nact - 1)];
        L[u] = partial ? partial_L(li, lj) : 1.0;
      }
#pragma unroll R == 1 ? 2 : 1
      for (int k = 0; k < napp; k++) {
        const double* Wk = Wall + (long)k * R * nW;
        double ki[R];
        onepass_gains<R>(Wk, nW, ir, Sinv + R * R * k, ki);
#pragma unroll
        for (int u = 0; u < UN; u++) {
          double wj[R];
          onepass_row<R>(Wk, nW, min(j0 + u, nact - 1), wj);
          p[u] = onepass_downdate<R>(p[u], L[u], ki, wj);
        }
      }
#pragma unroll
      for (int u = 0; u < UN; u++)
        if (ok[u]) P[i + (long)(j0 + u) * ld] = p[u];
    }
  }
}

// The epilogue behind the chain's last barrier, for a filter some entry of which got as far as touching x or P(rho, rho): x
// goes back, the rho diagonals (with nothing applied: those fix_depth edited and no other) and the status bits.
template <int T>
__device__ __forceinline__ void onepass_store(const StreamArgs& a, int b, double* xg, double* __restrict__ P, int len, int napp,
                                              unsigned flag, const double* xs, const double* D) {
  const int tid = threadIdx.x, ld = a.ld;
  for (int i = tid; i < xZ + 5 * len; i += T) xg[i] = xs[i];
  for (int f = tid; f < len; f += T) {
    const long dR = dxZ + 3 * f + 2;
    if (napp > 0 || __double_as_longlong(P[dR + dR * ld]) != __double_as_longlong(D[f])) P[dR + dR * ld] = D[f];
  }
  if (flag) atomicOr(&a.flags[b], flag);
}

}  // namespace viekf
