// viekf_capi_diag.hpp -- the entry points of the consistency diagnostics (include/viekf_diag.h; kernels in
// viekf_kernels_diag.hpp): read-only, the lower triangle of P only.  Their one buffer, the workspace of the batches whose packed
// triangle does not fit the LDS, belongs to the batch's owner.  Included by viekf_capi.hip ONLY, like viekf_dispatch.hpp.
#pragma once
#include "../../include/viekf_diag.h"
#include "viekf_dispatch.hpp"
#include "viekf_kernels_diag.hpp"
#include "viekf_staging.hpp"

extern "C" {

int viekf_diag_consistency(viekf_batch* b, const double* x_true, double* logdet, double* nees, double* whitened, int32_t* info,
                           viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!logdet && !nees && !whitened && !info) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (!x_true && (nees || whitened)) return fail(VIEKF_ERR_INVALID, "nees and whitened need x_true");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;
  const size_t B = (size_t)b->B;
  const double* d_xt = nullptr;
  double *d_ld = nullptr, *d_ne = nullptr, *d_wh = nullptr;
  int32_t* d_info = nullptr;
  Staged st(b, where);   // (four outputs; Staged keeps track of kMaxOut, viekf_staging.hpp)
  if (int rc = st.begin(in(x_true, B * b->nx, &d_xt), out(logdet, B, &d_ld), out(nees, 4 * B, &d_ne), out(whitened, B * b->n, &d_wh),
                        out(info, B, &d_info)))
    return rc;
  StreamArgs a = make_args(b);
  const size_t lds = sizeof(double) * (size_t)diag_packed_doubles(b->n);
  if (lds + 1024 <= 160 * 1024) {   // the packed triangle in LDS (N <= VIEKF_DIAG_ONCHIP_MAX_FEATURES; + the kernel's static LDS)
    static size_t have[64] = {};
    if (int rc = raise_dyn_lds({&k_diag_consistency<DG_T, true>}, lds, have[b->device & 63])) return rc;
    hipLaunchKernelGGL((k_diag_consistency<DG_T, true>), dim3(b->B), dim3(DG_T), lds, b->stream, a, 0, d_xt, nullptr, 0L, d_ld, d_ne,
                       d_wh, d_info);
    HIP_TRY(hipGetLastError());
  } else {                          // the same algorithm on a copy in the batch's workspace, a chunk of filters per launch
    const size_t stride = ((size_t)diag_packed_doubles(b->n) + 1) & ~size_t(1), per = sizeof(double) * stride;
    const size_t chunk = std::min(B, std::max<size_t>(1, (size_t(256) << 20) / per));
    if (int rc = b->own.reserve(&b->d_diag_ws, &b->diag_ws_cap, chunk * stride, b->stream)) return rc;
    for (size_t b0 = 0; b0 < B; b0 += chunk) {   // (launches of one stream: the next chunk reuses the workspace after this one)
      hipLaunchKernelGGL((k_diag_consistency<DG_T, false>), dim3((unsigned)std::min(chunk, B - b0)), dim3(DG_T), 0, b->stream, a, (int)b0,
                         d_xt, b->d_diag_ws, (long)stride, d_ld, d_ne, d_wh, d_info);
      HIP_TRY(hipGetLastError());
    }
  }
  return st.finish();
}

int viekf_diag_innovation(viekf_batch* b, int32_t type, int32_t M, const double* z, int32_t zdim, const int32_t* slot, const double* R,
                          int32_t rdim, int32_t r_mode, double* nis, double* residual, double* S, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!z || !R || !nis) return fail(VIEKF_ERR_INVALID, "z, R and nis must not be null");
  if (type < 0 || type >= VIEKF_TOTAL_MEAS || type == VIEKF_PIXEL_VEL)
    return fail(VIEKF_ERR_UNSUPPORTED, "measurement type not supported (PIXEL_VEL is an empty TODO in the reference)");
  if (zdim < 1 || zdim > 4 || rdim < 1 || rdim > 3 || r_mode < 0 || r_mode > 2)
    return fail(VIEKF_ERR_INVALID, "need 1 <= zdim <= 4, 1 <= rdim <= 3, r_mode 0, 1 or 2");
  if ((type == VIEKF_ATT || type == VIEKF_QZETA) && zdim != 4) return fail(VIEKF_ERR_INVALID, "ATT and QZETA take a quaternion: zdim 4");
  const bool needs_slot = type == VIEKF_QZETA || type == VIEKF_FEAT || type == VIEKF_DEPTH || type == VIEKF_INV_DEPTH;
  if (M < 1) return fail(VIEKF_ERR_INVALID, "M must be >= 1");
  if (needs_slot && !slot) return fail(VIEKF_ERR_INVALID, "slot must not be null for feature measurements");
  if (!needs_slot && (M != 1 || slot)) return fail(VIEKF_ERR_INVALID, "this measurement model takes M == 1 and no slot");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;
  const size_t BM = (size_t)b->B * (size_t)M, rr = (size_t)rdim * rdim;
  const double *d_z = nullptr, *d_R = nullptr;
  const int32_t* d_slot = nullptr;
  double *d_nis = nullptr, *d_res = nullptr, *d_S = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(z, BM * zdim, &d_z), in(slot, BM, &d_slot), in(R, r_count(b, M, r_mode, rr), &d_R),
                        out(nis, BM, &d_nis), out(residual, 3 * BM, &d_res), out(S, 9 * BM, &d_S)))
    return rc;
  StreamArgs a = make_args(b);
  const long rsb = r_mode == 1 ? (long)rr : (r_mode == 2 ? (long)rr * M : 0L), rsm = r_mode == 2 ? (long)rr : 0L;
  hipLaunchKernelGGL(k_diag_innovation, dim3((unsigned)((BM + 63) / 64)), dim3(64), 0, b->stream, a, type, M, d_z, zdim, d_slot, d_R,
                     rdim, rsb, rsm, d_nis, d_res, d_S);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

}  // extern "C"
