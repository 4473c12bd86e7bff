// viekf_kernels_util.hpp -- small kernels on P and on the per-filter bookkeeping: symmetrise, mirror the lower triangle up, read
// the diagonal or a block, copy filters between the live buffers and the ring, set the per-filter slot map.  Defines kernels:
// included from viekf_dispatch.hpp only.
#pragma once
#include "viekf_kernel_args.hpp"

namespace viekf {

// P <- (P + P^T) / 2 of every filter (a covariance handed in through viekf_batch_set_state): the kernels keep P exactly
// symmetric from then on and rely on it.  A NaN in the active block of the P handed in raises VIEKF_FLAG_NAN: the kernels only
// test x for NaN, and the reference's NaNsInTheHouse (vi_ekf_error.cpp:6-18) tests P as well.
__global__ void k_symmetrize(StreamArgs a) {
  const int b = blockIdx.y;
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B || e >= (long)a.n * a.n) return;
  const int i = (int)(e % a.n), j = (int)(e / a.n);
  if (i < j) return;
  double* P = a.P + a.si(b) * a.n * a.ld;
  const double v = i == j ? P[i + (long)i * a.ld] : 0.5 * (P[i + (long)j * a.ld] + P[j + (long)i * a.ld]);
  if (i > j) {
    P[i + (long)j * a.ld] = v;
    P[j + (long)i * a.ld] = v;
  }
  if (v != v && i < dxZ + 3 * a.len[b]) atomicOr(&a.flags[b], FLAG_NAN);
}

// upper triangle <- lower triangle (bit for bit), 32 x 32 tiles through LDS so that both sides are coalesced along the rows.
// Runs when a grouped update left the upper triangle stale (k_update_feat_blocked) and something is about to read all of P.
__global__ __launch_bounds__(256) void k_mirror_upper(StreamArgs a) {
  __shared__ double t[32][33];
  const int b = blockIdx.y, n = a.n, nt = (n + 31) >> 5;
  // tile pairs (ti >= tj) numbered row by row: blockIdx.x = ti (ti + 1) / 2 + tj
  int ti = (int)((sqrtf(1.0f + 8.0f * (float)blockIdx.x) - 1.0f) * 0.5f);
  while (ti * (ti + 1) / 2 > (int)blockIdx.x) ti--;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ti++;
  const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
  if (ti >= nt) return;
  double* P = a.P + a.si(b) * n * a.ld;
  const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
  for (int c = ly; c < 32; c += 8) {
    const int i = 32 * ti + lx, j = 32 * tj + c;
    t[c][lx] = (i < n && j < n) ? P[i + (long)j * a.ld] : 0.0;
  }
  __syncthreads();
  for (int c = ly; c < 32; c += 8) {
    const int i = 32 * tj + lx, j = 32 * ti + c;     // destination element (i, j) = source element (j, i)
    if (i < n && j < n && i < j) P[i + (long)j * a.ld] = t[lx][c];   // (a diagonal tile: its strictly upper part only)
  }
}

__global__ void k_cov_diag(StreamArgs a, double* __restrict__ out) {
  const int b = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < a.B && i < a.n) out[(long)b * a.n + i] = a.P[a.si(b) * a.n * a.ld + i + (long)i * a.ld];
}

// per-filter history: copies (x, P) of filter b between the batch's live buffers and ring slot slot[b] (< 0: filter skipped);
// to_ring != 0: live -> ring.  Filters on independent clocks advance and rewind their rings separately (viekf_seq, independent
// mode); the feature counts are not part of a slot, as in the reference's ring (include/vi_ekf.h:156-160).
__global__ __launch_bounds__(256) void k_ring_copy(StreamArgs a, double* __restrict__ ring_x, double* __restrict__ ring_P,
                                                   const int* __restrict__ slot, int to_ring, int depth) {
  const int b = blockIdx.x;
  if (b >= a.B) return;
  const int sl = slot[b];
  if (sl < 0) return;
  if (sl >= depth) {   // (a device-resident slot list cannot be validated by the host: nothing is copied, the filter is flagged)
    if (threadIdx.x == 0) atomicOr(&a.flags[b], FLAG_INTERNAL);
    return;
  }
  const long nP = (long)a.n * a.ld;
  double* lx = a.x + a.si(b) * a.nxs;
  double* lP = a.P + a.si(b) * nP;
  double* rx = ring_x + ((long)sl * a.B + b) * a.nxs;
  double* rP = ring_P + ((long)sl * a.B + b) * nP;
  const double2* src = reinterpret_cast<const double2*>(to_ring ? lP : rP);   // (ld is even and the buffers 16-byte aligned)
  double2* dst = reinterpret_cast<double2*>(to_ring ? rP : lP);
  for (long e = threadIdx.x; e < nP / 2; e += 256) dst[e] = src[e];
  for (int e = threadIdx.x; e < a.nxs; e += 256) (to_ring ? rx : lx)[e] = (to_ring ? lx : rx)[e];
}

// per-filter live slots: smap[b] = slot[b] * B + b for the filters with slot[b] >= 0 (viekf_batch_select_filters: the rewind of
// filters on clocks of their own is this index, vi_ekf_meas.cpp:50-52 per filter)
__global__ __launch_bounds__(256) void k_set_smap(int* __restrict__ smap, const int* __restrict__ slot, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b < B && slot[b] >= 0) smap[b] = slot[b] * B + b;
}

// a rectangular block P[r0 .. r0+nr, c0 .. c0+nc) of every filter -> out [B][nc][nr] (column-major per filter)
__global__ void k_cov_block(StreamArgs a, int r0, int c0, int nr, int nc, double* __restrict__ out) {
  const int b = blockIdx.y, e = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B || e >= nr * nc) return;
  const int c = e / nr, r = e - c * nr;
  out[(long)b * nr * nc + e] = a.P[a.si(b) * a.n * a.ld + (r0 + r) + (long)(c0 + c) * a.ld];
}

}  // namespace viekf
