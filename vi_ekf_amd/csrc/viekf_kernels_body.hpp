// viekf_kernels_body.hpp -- the body-sensor updates of one tick (ACC, ALT, ATT, POS, VEL: what the reference's imu_callback and
// truth_callback hand to VIEKF::update, vi_ekf_ros.cpp:172-199 / :452-470) in ONE pass over P.  Defines a kernel: included
// from viekf_dispatch.hpp only.
#pragma once
#include "viekf_body_lds.hpp"
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"
#include "viekf_onepass.hpp"

namespace viekf {

// One entry of the chain in 8 bits of the launch's `codes` word (entry m in bits 8 m ..): type | rdim << 4 | (zdim - 1) << 6.
// (Not arrays in the kernel arguments: indexing a by-value kernarg array by the loop counter spills it to scratch.)
__host__ __device__ constexpr unsigned long long body_code(int type, int zdim, int rdim) {
  return (unsigned long long)(type | rdim << 4 | (zdim - 1) << 6);
}

// The trailing pass of k_update_body_n for NA applied entries: columns 16 .. nact - 1 of the lower triangle, rho diagonals
// excepted.  A lane keeps ROW i (64 consecutive rows per wave: a column's segment is 512 contiguous bytes) with its gains in
// registers; the waves share the columns j <= i of a row block between them, UN of them in flight; W_m[j] and lambda_j are LDS
// broadcasts.  No division per element: the one remainder per lane and row block tells a rho row.
template <int T, int NA>
__device__ __forceinline__ void body_trailing(double* __restrict__ P, int ld, int nact, int n, int WL, bool partial,
                                              const double* Kall, const double* Wall, const double* lam) {
  constexpr int NW = T / 64;   // waves
  constexpr int UN = 8;        // columns a wave has in flight (the pass waits on memory: loads before arithmetic)
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int r0 = 0; r0 < nact; r0 += 64) {
    const int i = r0 + lane;
    const bool valid = i < nact;
    const int ir = valid ? i : 0;
    double kr[NA][3];
#pragma unroll
    for (int s = 0; s < NA; s++)
      for (int q = 0; q < 3; q++) kr[s][q] = Kall[3L * n * s + 3 * ir + q];
    const double li = lam[ir];
    const bool isrho = i >= dxZ && (i - dxZ) % 3 == 2;
    const int jend = min(r0 + 63, nact - 1);
    for (int j0 = dxZ + wid; j0 <= jend; j0 += NW * UN) {
      double p[UN];
      bool ok[UN];
#pragma unroll
      for (int u = 0; u < UN; u++) {
        const int j = j0 + u * NW;
        ok[u] = valid && j <= i && !(i == j && isrho);
        if (ok[u]) p[u] = P[i + (long)j * ld];
      }
#pragma unroll
      for (int u = 0; u < UN; u++) {
        const int j = j0 + u * NW;
        if (!ok[u]) continue;
        const double L = partial ? partial_L(li, lam[j]) : 1.0;
        const double* Wj = Wall + WL * j;
        double v = p[u];
#pragma unroll
        for (int s = 0; s < NA; s++) {
          double t = 0.0;
          for (int q = 0; q < 3; q++) t += kr[s][q] * Wj[3 * s + q];   // (K and W are zero past the entry's rdim)
          v -= L * t;
        }
        P[i + (long)j * ld] = v;
      }
    }
  }
}

// What an entry of the chain reports besides the status bits it raises (FLAG_*, the low bits of the same word).
constexpr unsigned kBodyDirty = 1u << 16;     // it touched x or a P(rho, rho)
constexpr unsigned kBodyApplied = 1u << 17;   // its K and W took slot `napp` and are due in the trailing pass

// Entry m of the chain for the workgroup's filter b, on the LDS image: the rules of k_update_generic in its order.
// (A function of its own, not inlined: inside the kernel's loop over the entries the compiler keeps values of every phase
//  live across the whole loop body -- more than 256 VGPRs, 83 spilled at a bound of 168; on its own it fits the 168 that three
//  waves per SIMD leave, with none spilled.)
template <int T>
__device__ __attribute__((noinline)) unsigned body_entry(const StreamArgs& a, int M, int m, int code, int b, int napp, double* smem,
                                                         const double* __restrict__ z_all, const double* __restrict__ R_all,
                                                         long r_stride_m, long r_stride_b,
                                                         const unsigned char* __restrict__ active_all, int* __restrict__ result_all) {
  constexpr int CL = kBodyPanelLd;
  const int WL = 3 * M;
  const int tid = threadIdx.x, n = a.n;
  const DevParams& prm = a.prm(uniform_filter(b));
  const BodyLds lds(a.nxs, n, M);
  double* xs = smem + lds.xs;
  double* lam = smem + lds.lam;
  double* Cp = smem + lds.C;
  double* D = smem + lds.D;
  double* Kall = smem + lds.K;
  double* Wall = smem + lds.W;
  double* sm = smem + lds.sm;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const int nxa = xZ + 5 * len;
  const bool partial = prm.use_partial_update != 0;
  unsigned st = 0;
  const int type = code & 15, rdim = (code >> 4) & 3, zdim = (code >> 6) + 1;
  const int act = active_all ? active_all[(long)m * a.B + b] : 1;
  int* res_out = result_all ? &result_all[(long)m * a.B + b] : nullptr;
  if (act == 2) { if (res_out && tid == 0) *res_out = -1; return st; }   // this filter skips the entry
  const double* z = z_all + ((long)m * a.B + b) * 4;
  {
    bool isnan_ = false;
    for (int i = 0; i < zdim; i++) isnan_ |= z[i] != z[i];
    if (isnan_) { if (res_out && tid == 0) *res_out = 2; return st; }   // MEAS_NAN
  }
  __syncthreads();   // what the load or the entry before wrote (xs, C, D); sm is free again
  if (act == 0) {    // :230 -- an inactive measurement only runs fix_depth
    for (int f = tid; f < len; f += T) fix_depth_diag(xs, D, f, prm, st);
    if (res_out && tid == 0) *res_out = 0;
    st |= kBodyDirty;
    return st;
  }
  if (tid == 0) {   // measurement model: zhat, the non-zero columns of H, residual
    int cols[6]; double Hc[18]; int nc = 0; double zhat[4] = {0, 0, 0, 0}; double r3[3] = {0, 0, 0};
    meas_model(type, xs, 0, prm, zhat, cols, Hc, nc);
    meas_residual(type, z, zhat, zdim, r3);
    for (int i = 0; i < 6; i++) sm[i] = (i < nc) ? (double)cols[i] : 0.0;
    for (int i = 0; i < 18; i++) sm[6 + i] = Hc[i];
    sm[24] = r3[0]; sm[25] = r3[1]; sm[26] = r3[2]; sm[27] = (double)nc;
  }
  __syncthreads();
  const int nc = (int)sm[27];
  double* W = Wall + 3 * napp;   // W_m[i][q] = W[WL * i + q]: row i holds every applied entry's three doubles side by side
  double* K = Kall + 3L * n * napp;
  // W = P H^T  (n x r): combination of the nc non-zero columns, all of them columns of the panel, in the model's order
  for (int i = tid; i < nact; i += T) {
    double w[3] = {0.0, 0.0, 0.0};
    for (int c = 0; c < nc; c++) {
      const double pv = Cp[CL * i + (int)sm[c]];
      for (int q = 0; q < rdim; q++) w[q] += pv * sm[6 + q * 6 + c];
    }
    for (int q = 0; q < 3; q++) W[WL * i + q] = w[q];
  }
  __syncthreads();
  if (tid == 0) {   // S = H W[cols] + R, inverse, gate
    const double* R = R_all + m * r_stride_m + b * r_stride_b;   // column-major rdim x rdim
    double S[9], Si[9];
    for (int p = 0; p < rdim; p++)
      for (int q = 0; q < rdim; q++) {
        double s = 0.0;
        for (int c = 0; c < nc; c++) s += sm[6 + p * 6 + c] * W[WL * (int)sm[c] + q];
        S[p * rdim + q] = s + R[p + q * rdim];
      }
    small_inverse_dev(rdim, S, Si);
    double mahal = 0.0;
    for (int q = 0; q < rdim; q++) { double t = 0.0; for (int p = 0; p < rdim; p++) t += sm[24 + p] * Si[p * rdim + q]; mahal += t * sm[24 + q]; }
    for (int i = 0; i < 9; i++) sm[28 + i] = (i < rdim * rdim) ? Si[i] : 0.0;
    sm[37] = (mahal > kGateMahal) ? 1.0 : 0.0;   // :234-239
  }
  __syncthreads();
  if (sm[37] != 0.0) { if (res_out && tid == 0) *res_out = 1; return st; }   // gated: no fix_depth, no slot taken
  int bad = 0;
  for (int i = tid; i < nact; i += T) {
    for (int q = 0; q < 3; q++) {
      double k = 0.0;
      if (q < rdim) for (int p = 0; p < rdim; p++) k += W[WL * i + p] * sm[28 + p * rdim + q];
      K[3 * i + q] = k;
      if (k != k) bad = 1;
    }
  }
  for (int i = 0; i < 18; i++) if (sm[6 + i] != sm[6 + i]) bad = 1;
  bad = __syncthreads_or(bad);
  if (!bad) {
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
      // P(rho, rho) of this feature
      const int dr = d + 2;
      double t = 0.0;
      for (int q = 0; q < rdim; q++) t += K[3 * dr + q] * W[WL * dr + q];
      D[f] -= (partial ? partial_L(lam[dr], lam[dr]) : 1.0) * t;
    }
    // the panel: the next entry's W comes from here
    for (int i = tid; i < nact; i += T) {
      const double li = lam[i];
#pragma unroll 2
      for (int c = 0; c < kBodyCols; c++) {
        const int hi = max(i, c), lo = min(i, c);   // (exactly symmetric, as k_update_generic)
        double t = 0.0;
        for (int q = 0; q < rdim; q++) t += K[3 * hi + q] * W[WL * lo + q];
        Cp[CL * i + c] -= (partial ? partial_L(li, lam[c]) : 1.0) * t;
      }
    }
    st |= kBodyApplied;   // K and W of this entry stay for the trailing pass
  }
  __syncthreads();
  for (int f = tid; f < len; f += T) fix_depth_diag(xs, D, f, prm, st);
  __syncthreads();
  for (int i = tid; i < nxa; i += T) {   // the scan k_update_generic makes when it writes x back
    const double v = xs[i];
    if (v != v) st |= FLAG_NAN;
    if (v > 1e6) st |= FLAG_BLOWUP;
  }
  if (res_out && tid == 0) *res_out = 0;
  st |= kBodyDirty;
  return st;
}

// ------------------------------------------------------------------------------------------------
// M body measurements, applied in order, with the arithmetic of M launches of k_update_generic -- element for element -- and
// one read and one write of the lower triangle of P.
//
// h_acc / h_alt / h_att / h_pos / h_vel are zero outside the 16 body columns, so W_m = P H_m^T is a combination of columns of
// the PANEL C = P[:, 0:16] alone: the whole chain -- model, W, S, gate, K, state correction -- runs on the panel in LDS, and
// the panel is the only part of P an entry has to bring up to date for the next one.  fix_depth edits P(rho, rho) of a
// feature, which later entries only subtract from: those diagonals ride along in D.  Every other element of the lower triangle
// takes no part in the chain; it gets the downdates  P_ij -= L_ij (K_m,i . W_m,j)  of the applied entries, in entry order,
// in the trailing pass: loaded once, stored once.  Nothing above the diagonal, at or past row / column nact, or in the pad
// rows is read or written.
//
// One workgroup per filter; a.si(b) is followed.  Phases and the rules of an entry: include/viekf_body.h.
// ------------------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(T, 3) void k_update_body_n(StreamArgs a, int M, unsigned long long codes,
                                                     const double* __restrict__ z_all,   // [M][B][4]
                                                     const double* __restrict__ R_all, long r_stride_m, long r_stride_b,
                                                     const unsigned char* __restrict__ active_all,   // [M][B] or NULL
                                                     int* __restrict__ result_all) {                 // [M][B] or NULL
  static_assert(T % 64 == 0, "whole waves");
  constexpr int CL = kBodyPanelLd;
  const int WL = 3 * M;            // row stride of W
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int n = a.n, ld = a.ld;
  const DevParams& prm = a.prm(b);
  const BodyLds lds(a.nxs, n, M);
  double* xs = smem + lds.xs;
  double* lam = smem + lds.lam;
  double* Cp = smem + lds.C;
  double* D = smem + lds.D;
  double* Kall = smem + lds.K;
  double* Wall = smem + lds.W;
  double* sm = smem + lds.sm;
  double* xg = a.x + a.si(b) * a.nxs;
  double* P = a.P + a.si(b) * n * ld;
  const int len = a.len[b];
  const int nact = 16 + 3 * len;
  const int nxa = xZ + 5 * len;
  const bool partial = prm.use_partial_update != 0;

  // ---- load: x, lambda, the panel (lower triangle only: row i of column c, or its mirror image), the rho diagonals ----
  for (int i = tid; i < nxa; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lam(b)[i];
  for (int i = tid; i < nact; i += T) {
#pragma unroll
    for (int c = 0; c < kBodyCols; c++) Cp[CL * i + c] = (i >= c) ? P[i + (long)c * ld] : P[c + (long)i * ld];
  }
  for (int f = tid; f < len; f += T) { const long dR = dxZ + 3 * f + 2; D[f] = P[dR + dR * ld]; }

  // ---- chain ----
  unsigned flag = 0;
  int napp = 0;         // entries applied so far: the slot of K / W the next one writes
  bool dirty = false;   // some entry got as far as touching x or P(rho, rho)
  for (int m = 0; m < M; m++) {
    const unsigned st = body_entry<T>(a, M, m, (int)((codes >> (8 * m)) & 0xffu), b, napp, smem, z_all, R_all, r_stride_m, r_stride_b,
                                      active_all, result_all);
    flag |= st & 0xffffu;
    dirty |= (st & kBodyDirty) != 0;
    napp += (st & kBodyApplied) ? 1 : 0;
  }
  if (!dirty) return;   // every entry skipped, NaN or gated: the filter is left as it is
  __syncthreads();
  for (int i = tid; i < nxa; i += T) xg[i] = xs[i];
  for (int f = tid; f < len; f += T) { const long dR = dxZ + 3 * f + 2; P[dR + dR * ld] = D[f]; }
  if (flag) atomicOr(&a.flags[b], flag);
  if (napp == 0) return;   // (fix_depth only: nothing else of P changed)

  // ---- the panel back: its lower triangle ----
  for (int i = tid; i < nact; i += T) {
#pragma unroll
    for (int c = 0; c < kBodyCols; c++)
      if (i >= c) P[i + (long)c * ld] = Cp[CL * i + c];
  }

  // ---- trailing pass ----
  switch (napp) {   // (the count as a template argument: the gains of a row sit in registers, no guard per entry)
    case 1: body_trailing<T, 1>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    case 2: body_trailing<T, 2>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    case 3: body_trailing<T, 3>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    case 4: body_trailing<T, 4>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    case 5: body_trailing<T, 5>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    case 6: body_trailing<T, 6>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    case 7: body_trailing<T, 7>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
    default: body_trailing<T, 8>(P, ld, nact, n, WL, partial, Kall, Wall, lam); break;
  }
}

// The M-launch route of viekf_batch_update_body: k_update_generic reads z as [B][zdim]; the call's cells are 4 doubles wide.
__global__ __launch_bounds__(256) void k_body_pack_z(int B, int zdim, const double* __restrict__ z4, double* __restrict__ zp) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  for (int i = 0; i < zdim; i++) zp[(long)b * zdim + i] = z4[(long)b * 4 + i];
}

}  // namespace viekf
