// viekf_kernels_depth.hpp -- the DEPTH (or INV_DEPTH) updates of one camera frame (what color_image_callback queues behind every
// FEAT it queued, vi_ekf_ros.cpp:287-305, handed to VIEKF::update) in ONE pass over P, the gather / scatter kernels of the
// M-launch route and the id -> slot lookup of the intake's depth step.  Defines kernels: included from viekf_dispatch.hpp only.
#pragma once
#include "viekf_depth_lds.hpp"
#include "viekf_kernel_args.hpp"
#include "viekf_meas_models.hpp"

namespace viekf {

// One applied entry's downdate of one element:  v -= L (K[hi] W[lo]),  K[hi] = W[hi] S^-1 -- operation by operation what
// k_update_generic does to P(i, j) with hi = max(i, j), lo = min(i, j) (its K, its t, its P -= L t).
__device__ __forceinline__ double depth_downdate(double v, double L, double whi, double wlo, double si) {
  double k = 0.0;
  k += whi * si;
  double t = 0.0;
  t += k * wlo;
  return v - L * t;
}

// The trailing pass of k_update_depths for napp applied entries: the lower triangle of the active block, rho diagonals excepted
// (they are stored from D).  A lane keeps ROW i (64 consecutive rows per wave: a column's segment is 512 contiguous bytes); a
// wave takes UN adjacent columns at a time, loads before arithmetic; per entry a lane reads its own W (one conflict-free read),
// S^-1 and the UN column values (broadcasts).  The entries run innermost, in order, on the values held in registers.
template <int T>
__device__ __forceinline__ void depth_trailing(double* __restrict__ P, int ld, int nact, int nW, int napp, bool partial,
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
        L[u] = partial ? (lj + li - li * lj) : 1.0;
      }
#pragma unroll 2
      for (int k = 0; k < napp; k++) {
        const double* Wk = Wall + (long)k * nW;
        const double wi = Wk[ir], si = Sinv[k];
#pragma unroll
        for (int u = 0; u < UN; u++) p[u] = depth_downdate(p[u], L[u], wi, Wk[min(j0 + u, nact - 1)], si);
      }
#pragma unroll
      for (int u = 0; u < UN; u++)
        if (ok[u]) P[i + (long)(j0 + u) * ld] = p[u];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// M DEPTH (TYPE = MT_DEPTH) or INV_DEPTH measurements per filter, applied in order, with the arithmetic of M launches of
// k_update_generic -- element for element -- and one read and one write of the lower triangle of P.
//
// h_depth / h_inv_depth have ONE non-zero element of H, at column c = 16 + 3 slot + 2: W = P H^T is that column of the
// current P times a scalar, S and K = W S^-1 follow from it.  The chain runs left-looking: the column an entry needs is the
// start P's column minus the downdates of the entries applied before it, which their W and S^-1 in LDS give
// (depth_downdate).  fix_depth edits P(rho, rho), which later entries only subtract from: those diagonals ride along in D,
// and the diagonal element of a column comes from D.  Every element of the lower triangle gets the downdates of the applied
// entries, in entry order, in the trailing pass: loaded once, stored once.  Nothing above the diagonal, at or past row /
// column nact, or in the pad rows is read or written.
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
  const DevParams& prm = *a.dp;
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
  const int nxa = xZ + 5 * len;
  const bool partial = prm.use_partial_update != 0;
  const long row = (long)b * M;
  auto entry_of = [&](int e) { return order ? M - 1 - e : e; };

  // ---- load: x, lambda, the rho diagonals, and for every entry the column of the start P its slot names (lower triangle only:
  //      row i of column c, or its mirror image) -- all of the chain's global loads, issued together ----
  for (int i = tid; i < nxa; i += T) xs[i] = xg[i];
  for (int i = tid; i < n; i += T) lam[i] = a.lambda[i];
  for (int f = tid; f < len; f += T) { const long dR = dxZ + 3 * f + 2; D[f] = P[dR + dR * ld]; }
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

  auto fix_depth_lds = [&](int f, unsigned& flag) {   // fix_depth_one with P(rho, rho) in D
    const int xR = xZ + 5 * f + 4;
    double rho = xs[xR];
    fix_depth_rule(rho, 1.0 / (2.0 * prm.min_depth), flag, [&](double e2) { D[f] += e2; }, [&] { D[f] = prm.P0_feat[2]; });
    xs[xR] = rho;
  };

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
      for (int f = tid; f < len; f += T) fix_depth_lds(f, flag);
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
      const double L = partial ? (lc + li - li * lc) : 1.0;
#pragma unroll 4   // (the reads of four entries in flight; the downdates stay in entry order)
      for (int k = 0; k < napp; k++) v = depth_downdate(v, L, Wall[(long)k * nW + hi], Wall[(long)k * nW + lo], Sinv[k]);
      if (i == c) v = D[slot];   // (the diagonal element is current in D, fix_depth's edits included)
      double w = 0.0;
      w += v * H;
      W[i] = w;
    }
    if (tid == 0) *badw = 0;
    __syncthreads();
    // S = H W[c] + R, inverse, gate (every thread: the verdict is uniform)
    const double R = R_all[b * r_stride_b + entry_of(e) * r_stride_m];
    double S, Si;
    {
      double s = 0.0;
      s += H * W[c];
      S = s + R;
    }
    small_inverse_dev(1, &S, &Si);
    double mahal = 0.0;
    { double t = 0.0; t += res * Si; mahal += t * res; }
    if (mahal > kGateMahal) { if (res_out) *res_out = 1; continue; }   // :234-239 gated: no fix_depth, no row taken
    int bad = (H != H) ? 1 : 0;
    for (int i = tid; i < nact; i += T) {
      double k = 0.0;
      k += W[i] * Si;
      if (k != k) bad = 1;
    }
    if (bad) *badw = 1;
    __syncthreads();
    bad = *badw;   // (the next writer of the word sits behind the next entry's first barrier)
    auto gain = [&](int i) { double k = 0.0; k += W[i] * Si; return k; };
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
      Sinv[napp] = Si;
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
        D[f] = depth_downdate(D[f], partial ? (lr + lr - lr * lr) : 1.0, W[dr], W[dr], Si);
      }
      fix_depth_lds(f, flag);
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
  for (int i = tid; i < nxa; i += T) xg[i] = xs[i];
  for (int f = tid; f < len; f += T) {   // (fix_depth only: the diagonals it edited and no other)
    const long dR = dxZ + 3 * f + 2;
    if (napp > 0 || __double_as_longlong(P[dR + dR * ld]) != __double_as_longlong(D[f])) P[dR + dR * ld] = D[f];
  }
  if (flag) atomicOr(&a.flags[b], flag);
  if (napp == 0) return;
  depth_trailing<T>(P, ld, nact, nW, napp, partial, Wall, Sinv, lam);
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

// viekf_frame_intake_depth: which entries of a frame are DEPTH measurements, and their slots.  One workgroup of 64 per filter.
//   slot_out [B][M]: the slot of the entry's id in the intake's table; -1 (viekf_batch_update_depths answers SKIPPED) for an
//   entry that is no measurement or a filter without a frame; kDepthNoSlot (>= every len_features: INVALID) for an id that is
//   not in the table, and for every id >= 0 of a filter whose table is stale.   act_out [B][M]: use_depth.
constexpr int kDepthNoSlot = 0x7fffffff;
__global__ __launch_bounds__(64) void k_frame_depth_plan(int B, int N, int M, const int* __restrict__ len, const int* __restrict__ tab,
                                                         const int* __restrict__ tlen, const int* __restrict__ ids,
                                                         const double* __restrict__ depth, const int* __restrict__ feat_result,
                                                         const unsigned char* __restrict__ active, int use_depth,
                                                         int* __restrict__ slot_out, unsigned char* __restrict__ act_out) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const bool act = active ? active[b] != 0 : true;
  const int tl = tlen[b];
  const bool stale = len[b] != tl;
  const int* row = tab + (long)b * N;
  for (int i = threadIdx.x; i < M; i += 64) {
    const long at = (long)b * M + i;
    const int id = ids[at];
    int slot = -1;
    if (act && id >= 0) {
      if (stale) slot = kDepthNoSlot;
      else {
        const int fr = feat_result[at];
        const double d = depth[at];
        if ((fr == 0 || fr == 1) && d == d && fabs(d) <= 1.7976931348623157e308) {   // queued as FEAT, finite depth
          slot = kDepthNoSlot;
          for (int f = 0; f < tl && f < N; f++)
            if (row[f] == id) { slot = f; break; }
        }
      }
    }
    slot_out[at] = slot;
    act_out[at] = use_depth ? (unsigned char)1 : (unsigned char)0;
  }
}

}  // namespace viekf
