// viekf_kernels_rec.hpp -- the device-resident flight recorder (include/viekf_rec.h): the estimated and the
// true pose of every filter on every frame, and the run judged on the device.
//
//   k_rec_push             one lane per filter: the frame's two poses, its validity, its channels.
//   k_rec_trajectory       one 256-thread workgroup per filter, lanes striding over the frames.  Pass 1: the centroids.  Pass
//                          2: the nine sums of A from CENTRED differences.  Lane 0: the alignment (viekf_rec_align.hpp).  Pass
//                          3: the ATE residuals and the RPE pairs.  A filter's two pose arrays are at most 458 KB, so passes 2
//                          and 3 read from L2.
//   k_rec_pose_ensemble    one workgroup per frame, lanes striding over the filters.
//   k_rec_channels_frame   one workgroup per frame, channel by channel, lanes striding over the filters (channels are stored
//                          time-major: the read is contiguous).
//   k_rec_channels_filter  one lane per (filter, channel), frames ascending (coalesced across filters).
// Storage: poses filter-major [B][cap][7] so that a filter's frames are contiguous for the three passes; validity [B][cap];
// channels time-major [cap][B][K].  fp64 throughout.  Every sum runs in a fixed order -- a lane's own elements ascending, the
// xor butterfly inside the wave, the waves through LDS in wave order -- and there is no atomic anywhere.
#pragma once
#include "viekf_kernel_args.hpp"
#include "viekf_rec_align.hpp"

namespace viekf {

constexpr int kRecThreads = 256, kRecWaves = kRecThreads / 64;

struct RecTabs {
  double* est;            // [B][cap][7]
  double* tru;            // [B][cap][7]
  unsigned char* valid;   // [B][cap]
  double* chan;           // [cap][B][K]
  int cap, K;
};

__device__ __forceinline__ double rec_nan() { return __longlong_as_double(0x7ff8000000000000LL); }
__device__ __forceinline__ bool rec_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (false for NaN)

// The sum (or the maximum) of NV values per lane over a 256-thread workgroup, in every lane: the butterfly inside the wave,
// then the waves in wave order.  lds: kRecWaves * NV doubles; free again when this returns.
template <int NV, bool MAX = false>
__device__ __forceinline__ void rec_block_reduce(double (&v)[NV], double* lds) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; i++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double o = __shfl_xor(v[i], off, 64);
      v[i] = MAX ? fmax(v[i], o) : v[i] + o;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NV; i++) lds[w * NV + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NV; i++) {
    double s = lds[i];
#pragma unroll
    for (int k = 1; k < kRecWaves; k++) s = MAX ? fmax(s, lds[k * NV + i]) : s + lds[k * NV + i];
    v[i] = s;
  }
  __syncthreads();
}

__device__ __forceinline__ void rec_load7(const double* __restrict__ p, double* o) {
#pragma unroll
  for (int i = 0; i < 7; i++) o[i] = p[i];
}

// T1^-1 * T2
__device__ __forceinline__ void rec_between(const double* T1, const double* T2, double* E) {
  const double d[3] = {T2[0] - T1[0], T2[1] - T1[1], T2[2] - T1[2]};
  const double qi[4] = {T1[3], -T1[4], -T1[5], -T1[6]};
  q_rotp(T1 + 3, d, E);
  q_otimes(qi, T2 + 3, E + 3);
}

// ---- kernels ----
// frame k of every filter.  chan [B][K] or null (K == 0); mask [B] or null.
__global__ __launch_bounds__(64) void k_rec_push(int B, RecTabs t, int k, const double* __restrict__ est_pose, const double* __restrict__ x_true,
                                                 int ldx, const double* __restrict__ chan, const unsigned char* __restrict__ mask) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double e[7], r[7];
  rec_load7(est_pose + (long)b * 7, e);
  const double* xt = x_true + (long)b * ldx;
#pragma unroll
  for (int i = 0; i < 3; i++) r[i] = xt[xPOS + i];
#pragma unroll
  for (int i = 0; i < 4; i++) r[3 + i] = xt[xATT + i];
  bool ok = !mask || mask[b] != 0;
#pragma unroll
  for (int i = 0; i < 7; i++) ok = ok && rec_finite(e[i]) && rec_finite(r[i]);
  const long at = ((long)b * t.cap + k) * 7;
#pragma unroll
  for (int i = 0; i < 7; i++) { t.est[at + i] = e[i]; t.tru[at + i] = r[i]; }
  t.valid[(long)b * t.cap + k] = ok ? 1 : 0;
  for (int j = 0; j < t.K; j++) t.chan[((long)k * B + b) * t.K + j] = chan[(long)b * t.K + j];
}

// ATE and RPE of filter blockIdx.x over first <= k < last; every output may be null
__global__ __launch_bounds__(kRecThreads) void k_rec_trajectory(RecTabs t, int align, int first, int last, int delta, double* __restrict__ ate_pos,
                                                                double* __restrict__ ate_att, double* __restrict__ rpe_pos,
                                                                double* __restrict__ rpe_att, double* __restrict__ align_pose,
                                                                int* __restrict__ n_used) {
  __shared__ double lds[kRecWaves * 9];
  __shared__ double s_al[7];
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* est = t.est + (long)b * t.cap * 7;
  const double* tru = t.tru + (long)b * t.cap * 7;
  const unsigned char* val = t.valid + (long)b * t.cap;

  // pass 1: n and the centroids
  double s1[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = first + tid; k < last; k += kRecThreads) {
    if (!val[k]) continue;
    s1[0] += 1.0;
#pragma unroll
    for (int i = 0; i < 3; i++) { s1[1 + i] += tru[(long)k * 7 + i]; s1[4 + i] += est[(long)k * 7 + i]; }
  }
  rec_block_reduce<7>(s1, lds);
  const double n = s1[0];
  const double ct[3] = {s1[1] / n, s1[2] / n, s1[3] / n}, ce[3] = {s1[4] / n, s1[5] / n, s1[6] / n};

  // pass 2: A = sum (p_t - c_t)(p_e - c_e)^T from the centred differences
  double A[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (align != 0) {   // (uniform over the launch)
    for (int k = first + tid; k < last; k += kRecThreads) {
      if (!val[k]) continue;
      double dt[3], de[3];
#pragma unroll
      for (int i = 0; i < 3; i++) { dt[i] = tru[(long)k * 7 + i] - ct[i]; de[i] = est[(long)k * 7 + i] - ce[i]; }
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) A[3 * i + j] += dt[i] * de[j];
    }
    rec_block_reduce<9>(A, lds);
  }

  // the alignment, by lane 0: {t_a, q_a}
  if (tid == 0) {
    double q[4] = {1.0, 0.0, 0.0, 0.0}, ta[3] = {0.0, 0.0, 0.0};
    if (align == 1) rec_align_yaw(A, q);
    if (align == 2) rec_align_se3(A, q);
    if (align != 0) {
      double rc[3];
      q_rota(q, ce, rc);
#pragma unroll
      for (int i = 0; i < 3; i++) ta[i] = ct[i] - rc[i];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) s_al[i] = ta[i];
#pragma unroll
    for (int i = 0; i < 4; i++) s_al[3 + i] = q[i];
  }
  __syncthreads();
  double al[7];
#pragma unroll
  for (int i = 0; i < 7; i++) al[i] = s_al[i];
  // p_t - (R_a p_e + t_a) = (p_t - c_t) - R_a (p_e - c_e) + off with off = c_t - R_a c_e - t_a: zero under an alignment, c_t - c_e
  // without one.  The centred form keeps its digits on a trajectory far from the origin.
  double off[3] = {0.0, 0.0, 0.0};
  if (align == 0) {
#pragma unroll
    for (int i = 0; i < 3; i++) off[i] = ct[i] - ce[i];
  }

  // pass 3: the ATE residuals and the RPE pairs
  double s3[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // sum |dp|^2, sum |dq|^2, pairs, sum |D.t|^2, sum |D.q|^2
  for (int k = first + tid; k < last; k += kRecThreads) {
    if (!val[k]) continue;
    double Te[7], Tt[7];
    rec_load7(est + (long)k * 7, Te);
    rec_load7(tru + (long)k * 7, Tt);
    double de[3], r[3], qa[4], dq[3];
#pragma unroll
    for (int i = 0; i < 3; i++) de[i] = Te[i] - ce[i];
    q_rota(al + 3, de, r);
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) { const double d = (Tt[i] - ct[i]) - r[i] + off[i]; d2 += d * d; }
    s3[0] += d2;
    q_otimes(al + 3, Te + 3, qa);
    q_boxminus_dev(Tt + 3, qa, dq);
    s3[1] += dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2];
    const int k2 = k + delta;
    if (k2 < last && val[k2]) {
      double Te2[7], Tt2[7], Ee[7], Et[7], D[7];
      rec_load7(est + (long)k2 * 7, Te2);
      rec_load7(tru + (long)k2 * 7, Tt2);
      rec_between(Te, Te2, Ee);
      rec_between(Tt, Tt2, Et);
      rec_between(Et, Ee, D);
      const double id[4] = {1.0, 0.0, 0.0, 0.0};
      q_boxminus_dev(D + 3, id, dq);
      s3[2] += 1.0;
      s3[3] += D[0] * D[0] + D[1] * D[1] + D[2] * D[2];
      s3[4] += dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2];
    }
  }
  rec_block_reduce<5>(s3, lds);
  if (tid == 0) {
    const double nan = rec_nan(), pairs = s3[2];
    if (ate_pos) ate_pos[b] = n > 0.0 ? sqrt(s3[0] / n) : nan;
    if (ate_att) ate_att[b] = n > 0.0 ? sqrt(s3[1] / n) : nan;
    if (rpe_pos) rpe_pos[b] = pairs > 0.0 ? sqrt(s3[3] / pairs) : nan;
    if (rpe_att) rpe_att[b] = pairs > 0.0 ? sqrt(s3[4] / pairs) : nan;
    if (align_pose) {
#pragma unroll
      for (int i = 0; i < 7; i++) align_pose[(long)b * 7 + i] = n > 0.0 ? al[i] : nan;
    }
    if (n_used) { n_used[2 * b] = (int)n; n_used[2 * b + 1] = (int)pairs; }
  }
}

// out [T'][4] = {n, rms |p_t - p_e|, rms |q_t [-] q_e|, max |p_t - p_e|} of frame first + blockIdx.x over the batch
__global__ __launch_bounds__(kRecThreads) void k_rec_pose_ensemble(int B, RecTabs t, int first, double* __restrict__ out) {
  __shared__ double lds[kRecWaves * 3];
  const int k = first + blockIdx.x, tid = threadIdx.x;
  double s[3] = {0.0, 0.0, 0.0}, mx[1] = {0.0};
  for (int b = tid; b < B; b += kRecThreads) {
    if (!t.valid[(long)b * t.cap + k]) continue;
    double Te[7], Tt[7], dq[3];
    rec_load7(t.est + ((long)b * t.cap + k) * 7, Te);
    rec_load7(t.tru + ((long)b * t.cap + k) * 7, Tt);
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) { const double d = Tt[i] - Te[i]; d2 += d * d; }
    q_boxminus_dev(Tt + 3, Te + 3, dq);
    s[0] += 1.0;
    s[1] += d2;
    s[2] += dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2];
    mx[0] = fmax(mx[0], d2);
  }
  rec_block_reduce<3>(s, lds);
  rec_block_reduce<1, true>(mx, lds);
  if (tid == 0) {
    const double nan = rec_nan(), n = s[0];
    double* o = out + (long)blockIdx.x * 4;
    o[0] = n;
    o[1] = n > 0.0 ? sqrt(s[1] / n) : nan;
    o[2] = n > 0.0 ? sqrt(s[2] / n) : nan;
    o[3] = n > 0.0 ? sqrt(mx[0]) : nan;
  }
}

// one value into {n, sum, below, above} and the running maximum; a value that is not finite is skipped
__device__ __forceinline__ void rec_chan_take(double v, bool has_lo, double lo, bool has_hi, double hi, double (&s)[4], double& mx, bool& any) {
  if (!rec_finite(v)) return;
  s[0] += 1.0;
  s[1] += v;
  s[2] += (has_lo && v < lo) ? 1.0 : 0.0;
  s[3] += (has_hi && v > hi) ? 1.0 : 0.0;
  mx = any ? fmax(mx, v) : v;
  any = true;
}
__device__ __forceinline__ void rec_chan_put(const double (&s)[4], double mx, double* o) {
  const double n = s[0], nan = rec_nan();
  o[0] = n;
  o[1] = n > 0.0 ? s[1] / n : nan;
  o[2] = n > 0.0 ? mx : nan;
  o[3] = n > 0.0 ? s[2] / n : 0.0;
  o[4] = n > 0.0 ? s[3] / n : 0.0;
}

// per_frame [T'][K][5] of frame first + blockIdx.x over the batch.  lo / hi [K] or null.
__global__ __launch_bounds__(kRecThreads) void k_rec_channels_frame(int B, RecTabs t, int first, const double* __restrict__ lo,
                                                                    const double* __restrict__ hi, double* __restrict__ out) {
  __shared__ double lds[kRecWaves * 4];
  const int k = first + blockIdx.x, tid = threadIdx.x;
  const double* row = t.chan + (long)k * B * t.K;
  for (int j = 0; j < t.K; j++) {
    const double lj = lo ? lo[j] : 0.0, hj = hi ? hi[j] : 0.0;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, mx[1] = {-1.7976931348623157e308};
    bool any = false;
    for (int b = tid; b < B; b += kRecThreads) rec_chan_take(row[(long)b * t.K + j], lo != nullptr, lj, hi != nullptr, hj, s, mx[0], any);
    rec_block_reduce<4>(s, lds);
    rec_block_reduce<1, true>(mx, lds);   // (a lane that saw nothing holds the lowest double)
    if (tid == 0) rec_chan_put(s, mx[0], out + ((long)blockIdx.x * t.K + j) * 5);
  }
}

// per_filter [B][K][5] of filter b (x) and channel blockIdx.y over first <= k < last, frames ascending
__global__ __launch_bounds__(64) void k_rec_channels_filter(int B, RecTabs t, int first, int last, const double* __restrict__ lo,
                                                            const double* __restrict__ hi, double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y;
  if (b >= B) return;
  const double lj = lo ? lo[j] : 0.0, hj = hi ? hi[j] : 0.0;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, mx = 0.0;
  bool any = false;
#pragma unroll 4
  for (int k = first; k < last; k++) rec_chan_take(t.chan[((long)k * B + b) * t.K + j], lo != nullptr, lj, hi != nullptr, hj, s, mx, any);
  rec_chan_put(s, mx, out + ((long)b * t.K + j) * 5);
}

}  // namespace viekf
