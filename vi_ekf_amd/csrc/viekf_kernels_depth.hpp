// viekf_kernels_depth.hpp -- the DEPTH (or INV_DEPTH) updates of one camera frame (what color_image_callback queues behind every
// FEAT it queued, vi_ekf_ros.cpp:287-305, handed to VIEKF::update) in ONE pass over P and the gather / scatter kernels of the
// M-launch route.  (The id -> slot lookup of the intake's depth step: k_frame_slot_plan, viekf_kernels_frame.hpp.)
// Defines kernels: included from viekf_dispatch.hpp only.
#pragma once
#include "viekf_depth_lds.hpp"
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"
#include "viekf_onepass.hpp"

namespace viekf {

// ------------------------------------------------------------------------------------------------
// M DEPTH (TYPE = MT_DEPTH) or INV_DEPTH measurements per filter, applied in order, with the arithmetic of M launches of
// k_update_generic -- element for element -- and one read and one write of the lower triangle of P.
//
// h_depth / h_inv_depth have ONE non-zero element of H, at column c = 16 + 3 slot + 2: W = P H^T is that column of the
// current P times a scalar, S and K = W S^-1 follow from it.  The chain runs left-looking: the column an entry needs is the
// start P's column minus the downdates of the entries applied before it, which their W and S^-1 in LDS give
// (onepass_rebuild<1>).  The rho diagonals in D, the trailing pass and what is never touched: viekf_onepass.hpp.
//
// One workgroup per filter; a.si(b) is followed.  The rules of an entry, in k_update_generic's order: include/viekf_depth.h.
// ------------------------------------------------------------------------------------------------
template <int T, int TYPE>
__global__ __launch_bounds__(T) void k_update_depths(StreamArgs a, int M, int order,
                                                     const int* __restrict__ slot_all,   // [B][M]
                                                     const double* __restrict__ z_all,   // [B][M]
                                                     const double* __restrict__ R_all, long r_stride_b, long r_stride_m,
                                                     const unsigned char* __restrict__ active_all,   // [B][M] or NULL
                                                     int* __restrict__ result_all) {                 // [B][M] or NULL
  static_assert(T % 64 == 0, "whole waves");
  static_assert(TYPE == MT_DEPTH || TYPE == MT_INV_DEPTH, "one non-zero element of H, at the feature's rho column");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n, ld = a.ld;
  const DevParams& prm = a.prm(b);
  const DepthLds lds(a.nxs, n, M);
  const int nW = lds.nW;
  double* xs = smem + lds.xs;
  double* lam = smem + lds.lam;
  double* D = smem + lds.D;
  double* Sinv = smem + lds.Si;
  int* badw = reinterpret_cast<int*>(smem + lds.bad);
  double* Wall = smem + lds.W;
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const bool partial = prm.use_partial_update != 0;
  const long row = (long)b * M;
  auto entry_of = [&](int e) { return order ? M - 1 - e : e; };

  // ---- load: x, lambda, the rho diagonals, and for every entry the column of the start P its slot names (lower triangle only:
  //      row i of column c, or its mirror image) -- all of the chain's global loads, issued together ----
  onepass_load<T>(a, b, xg, P, len, xs, lam, D);
  for (int i = tid; i < nact; i += T) {
    constexpr int UL = 8;   // columns a thread has in flight (the chain cannot start before the last of them is in)
    for (int e0 = 0; e0 < M; e0 += UL) {
      double v[UL];
      bool ok[UL];
#pragma unroll
      for (int u = 0; u < UL; u++) {
        const int e = e0 + u;
        const int slot = e < M ? slot_all[row + entry_of(e)] : -1;
        ok[u] = slot >= 0 && slot < len;
        const int c = dxZ + 3 * slot + 2;
        v[u] = 0.0;
        if (ok[u]) v[u] = (i >= c) ? P[i + (long)c * ld] : P[c + (long)i * ld];
      }
#pragma unroll
      for (int u = 0; u < UL; u++)
        if (ok[u]) Wall[(long)(e0 + u) * nW + i] = v[u];
    }
  }

  // ---- chain ----
  unsigned flag = 0;    // (per thread; ORed into the filter's word at the end)
  int napp = 0;         // entries applied so far: the row of W / Si the next one writes
  bool dirty = false;   // some entry got as far as touching x or P(rho, rho)
  for (int e = 0; e < M; e++) {
    const long at = row + entry_of(e);
    const int act = active_all ? active_all[at] : 1;
    int* res_out = (result_all && tid == 0) ? &result_all[at] : nullptr;
    if (act == 2) { if (res_out) *res_out = -1; continue; }   // this filter skips the entry
    const int slot = slot_all[at];
    if (slot < 0 || slot >= len) { if (res_out) *res_out = (slot < 0) ? -1 : 3; continue; }
    const double z = z_all[at];
    if (z != z) { if (res_out) *res_out = 2; continue; }   // MEAS_NAN
    __syncthreads();   // what the load or the entry before wrote (xs, D, W, Si)
    if (act == 0) {    // :230 -- an inactive measurement only runs fix_depth
      for (int f = tid; f < len; f += T) fix_depth_diag(xs, D, f, prm, flag);
      if (res_out) *res_out = 0;
      dirty = true;
      continue;
    }
    // measurement model, on every thread (one column, one element of H): zhat, H, residual
    int cols[6]; double Hc[18]; int nc = 0; double zhat[4] = {0, 0, 0, 0}; double r3[3] = {0, 0, 0};
    meas_model(TYPE, xs, slot, prm, zhat, cols, Hc, nc);
    meas_residual(TYPE, &z, zhat, 1, r3);
    const int c = cols[0];
    const double H = Hc[0], res = r3[0];
    // the column c of the current P, left-looking, and W = P H^T
    double* W = Wall + (long)napp * nW;
    const double lc = lam[c];
    for (int i = tid; i < nact; i += T) {
      double v = Wall[(long)e * nW + i];
      const int hi = max(i, c), lo = min(i, c);
      const double li = lam[i];
      const double L = partial ? partial_L(li, lc) : 1.0;
      v = onepass_rebuild<1, 4>(v, L, Wall, nW, Sinv, napp, hi, lo);   // (four entries' reads in flight)
      if (i == c) v = D[slot];   // (the diagonal element is current in D, fix_depth's edits included)
      double w = 0.0;
      w += v * H;
      W[i] = w;
    }
    if (tid == 0) *badw = 0;
    __syncthreads();
    // S = H W[c] + R, inverse, gate (every thread: the verdict is uniform)
    const double R = R_all[b * r_stride_b + entry_of(e) * r_stride_m];
    double S, Si[1];
    {
      double s = 0.0;
      s += H * W[c];
      S = s + R;
    }
    small_inverse_dev(1, &S, Si);
    double mahal = 0.0;
    { double t = 0.0; t += res * Si[0]; mahal += t * res; }
    if (mahal > kGateMahal) { if (res_out) *res_out = 1; continue; }   // :234-239 gated: no fix_depth, no row taken
    int bad = (H != H) ? 1 : 0;
    for (int i = tid; i < nact; i += T) {
      double k[1];
      onepass_gains<1>(W, nW, i, Si, k);
      if (k[0] != k[0]) bad = 1;
    }
    if (bad) *badw = 1;
    __syncthreads();
    bad = *badw;   // (the next writer of the word sits behind the next entry's first barrier)
    auto gain = [&](int i) { double k[1]; onepass_gains<1>(W, nW, i, Si, k); return k[0]; };
    if (!bad && tid == 0) {
      double dxb[16], xo[17];
      for (int i = 0; i < 16; i++) {
        const double l = partial ? lam[i] : 1.0;
        double s = 0.0;
        s += (l * gain(i)) * res;
        dxb[i] = s;
      }
      body_boxplus(xs, dxb, xo);
      for (int i = 0; i < 17; i++) xs[i] = xo[i];
      Sinv[napp] = Si[0];
    }
    // a thread's features: correction, P(rho, rho), fix_depth and the scan k_update_generic makes when it writes x back
    for (int f = tid; f < len; f += T) {
      double* xf = xs + xZ + 5 * f;
      if (!bad) {
        const int d = 16 + 3 * f;
        double dv[3];
        for (int q = 0; q < 3; q++) {
          const double l = partial ? lam[d + q] : 1.0;
          double s = 0.0;
          s += (l * gain(d + q)) * res;
          dv[q] = s;
        }
        double qn[4];
        q_feat_boxplus(xf, dv[0], dv[1], qn);
        xf[0] = qn[0]; xf[1] = qn[1]; xf[2] = qn[2]; xf[3] = qn[3];
        xf[4] += dv[2];
        const int dr = d + 2;
        const double lr = lam[dr];
        D[f] = onepass_apply<1>(D[f], partial ? partial_L(lr, lr) : 1.0, W, nW, Si, dr, dr);
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
  onepass_trailing<T, 1>(P, ld, nact, nW, napp, partial, Wall, Sinv, lam);
}

// The M-launch route of viekf_batch_update_depths: entry m of every filter in the [B] rows k_update_generic reads ...
__global__ __launch_bounds__(256) void k_depths_gather(int B, int M, int m, const int* __restrict__ slot, const double* __restrict__ z,
                                                       const double* __restrict__ R2, const unsigned char* __restrict__ active,
                                                       int* __restrict__ slot_m, double* __restrict__ z_m, double* __restrict__ R_m,
                                                       unsigned char* __restrict__ act_m) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const long at = (long)b * M + m;
  slot_m[b] = slot[at];
  z_m[b] = z[at];
  if (R2) R_m[b] = R2[at];
  act_m[b] = active ? active[at] : (unsigned char)1;
}

// ... and its result codes back into the call's [B][M]
__global__ __launch_bounds__(256) void k_depths_scatter(int B, int M, int m, const int* __restrict__ res_m, int* __restrict__ result) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  result[(long)b * M + m] = res_m[b];
}

}  // namespace viekf
