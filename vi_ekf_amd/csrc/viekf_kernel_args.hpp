// viekf_kernel_args.hpp -- what every kernel of the library takes and shares: the argument struct (StreamArgs), the carve-up of
// the per-filter global workspace (WsLayout), the MFMA operand type and contraction depth, the wave-level LDS fence and
// fix_depth on a filter's state.  Defines NO __global__ function: any header and any translation unit may include it.
#pragma once
#include "viekf_device.hpp"
#include "viekf_fastmath.hpp"

namespace viekf {

struct StreamArgs {
  double* x;            // [B][nxs]
  double* P;            // [B][n][ld]
  int* len;             // [B]
  unsigned* flags;      // [B]
  const double* Qx;     // [n] diagonal, or [B][n] (pstride = 1); read through qx(b) only
  const double* lambda; // [n], or [B][n]; read through lam(b) only
  double* ws;           // [B][ws_stride]
  int B, N, nx, nxs, n, ld;
  long ws_stride;
  const DevParams* dp;  // device memory (uniform loads); NOT by value: indexing a by-value kernarg array spills it to scratch
                        // one set, or [B] of them (pstride = 1); read through prm(b) only
  int pstride;          // 0: the batch's one parameter set; 1: one set per filter (viekf_batch_set_params_filters)
  double* x_out;        // where the fused-step kernel stores the state / covariance: the same buffers (in place) or another
  double* P_out;        // slot of the history ring (viekf_batch_propagate_to: the propagate writes the NEXT slot, no copy)
  const unsigned char* active;   // [B] or NULL: filters with active[b] == 0 take no part in a propagate / feature-update launch
                                 // (viekf_batch_set_active: filters on different clocks share a batch)
  const int* resmap;    // fused-step kernel: ownership map of the 3x3 feature blocks, [RB][TW] entries I | J << 8 | owned << 16
  // Per-filter live ring slots (viekf_batch_select_filters: filters on clocks of their own share a batch, each with its own ring
  // position): x / P then point at the RING, [slot][B] entries, and filter b's state is entry smap[b] = slot_b * B + b of it.
  // smap_out: where the fused kernel stores filter b's state (viekf_batch_propagate_filters_to: slot i_b -> slot i_b + 1, no copy).
  int* smap;            // (device memory; the fused kernel moves a filter's entry to smap_out[b] when it stores it there)
  const int* smap_out;
  // [B] or NULL: propagates of THIS launch per filter (viekf_batch_propagate_n_filters_to; >= 1 for every filter that takes part).
  // Read by the multi-propagate instances of the fused kernel only; NULL = the launch-wide count of the launch word.
  const int* kcount;
  // Filter b's parameter set.  With pstride == 0 every address is the shared set's.  b is the workgroup's filter wherever a
  // workgroup serves one filter, so the loads stay scalar; where the compiler cannot see that (two filters per workgroup) the
  // caller passes uniform_filter(b).
  __device__ __forceinline__ const DevParams& prm(int b) const { return dp[(long)b * pstride]; }
  __device__ __forceinline__ const double* qx(int b) const { return Qx + (long)b * pstride * n; }
  __device__ __forceinline__ const double* lam(int b) const { return lambda + (long)b * pstride * n; }
  __device__ __forceinline__ long si(int b) const { return smap ? (long)smap[b] : (long)b; }
  __device__ __forceinline__ long so(int b) const { return smap_out ? (long)smap_out[b] : si(b); }
};

// b as a value the compiler knows to be the same in every lane of the wave (the wave's filter): parameter loads indexed by it stay
// scalar loads
__device__ __forceinline__ int uniform_filter(int b) { return __builtin_amdgcn_readfirstlane(b); }

constexpr int WK = 40;   // contraction depth of the low-rank part (16 + 16 + 6, padded to whole MFMA k-steps of 4)
typedef double v4f64 __attribute__((ext_vector_type(4)));

// workspace carve-up (doubles) for one filter
struct WsLayout {
  long phi_fb, phi_ff, gd, U, pbr, pbc, Xw, Yw, total;
  __host__ __device__ WsLayout(int N, int n) {
    long o = 0;
    phi_fb = o; o += 3L * N * 16;   // [3N][16]
    phi_ff = o; o += 9L * N;        // [N][9]
    gd = o;     o += 6L * n;        // [n][6]
    U = o;      o += 3L * N * 16;   // [3N][16]   (Phi P)[feat rows, body cols]
    pbr = o;    o += 16L * n;       // [16][n]    copy of P[body rows, :]
    pbc = o;    o += 16L * n;       // [16][n]    copy of P[:, body cols], stored [k][i]
    const long nfp = ((3L * N + 47) / 48) * 48;
    Xw = o;     o += nfp * WK;      // [nfp][WK]  low-rank factors of the propagate's MFMA pass (k_propagate_stream<.., true>):
    Yw = o;     o += nfp * WK;      //            P+_ff = D P_ff D^T + Xw Yw^T, rows padded to whole 48-row super-tiles
    total = (o + 1) & ~1L;
  }
};

// fix_depth (vi_ekf_helper.cpp:128-156) for feature i of the block's filter; xs is the LDS copy of x
__device__ __forceinline__ void fix_depth_one(double* xs, double* P, int ld, int i, const DevParams& p, unsigned& flag) {
  const int xR = xZ + 5 * i + 4, dR = dxZ + 3 * i + 2;
  double rho = xs[xR];
  fix_depth_rule(rho, 1.0 / (2.0 * p.min_depth), flag, [&](double e2) { P[dR + (long)dR * ld] += e2; },
                 [&] { P[dR + (long)dR * ld] = p.P0_feat[2]; });
  xs[xR] = rho;
}

// LDS written by some lanes of a wave and read by others of the SAME wave: order the accesses (the compiler treats lanes as
// independent threads and may otherwise move the loads above the stores)
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace viekf
