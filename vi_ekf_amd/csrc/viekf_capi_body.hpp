// viekf_capi_body.hpp -- the fused body-sensor update (include/viekf_body.h; its kernel in viekf_kernels_body.hpp): the checks,
// the choice between the one fused launch and the M launches of k_update_generic, and the entry points.  Launches the batch's
// kernels through viekf_dispatch.hpp: included by viekf_capi.hip ONLY.
#pragma once
#include "../../include/viekf_body.h"
#include "viekf_body_lds.hpp"
#include "viekf_dispatch.hpp"
#include "viekf_staging.hpp"

static_assert(VIEKF_BODY_MAX_M == kBodyMaxM, "the header's limit is the kernel's");

namespace {

// what the device gives one workgroup
int body_lds_limit(int device, size_t* bytes) {
  int v = 0;
  HIP_TRY(hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device));
  *bytes = v > 0 ? (size_t)v : 0;
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int64_t viekf_body_lds_bytes(int32_t num_features, int32_t M) {
  int nxs = 0, n = 0;
  if (!lds_dims(num_features, &nxs, &n) || M < 1 || M > VIEKF_BODY_MAX_M) return 0;
  return (int64_t)BodyLds(nxs, n, M).bytes();
}

int viekf_body_lds_limit(int32_t device, int64_t* bytes) {
  if (!bytes) return fail(VIEKF_ERR_INVALID, "bytes must not be null");
  size_t v = 0;
  if (int rc = body_lds_limit(device, &v)) return rc;
  *bytes = (int64_t)v;
  return VIEKF_OK;
}

int viekf_batch_update_body(viekf_batch* b, int32_t M, const int32_t* types, const int32_t* zdim, const int32_t* rdim,
                            const double* z, const double* R, int32_t r_mode, const uint8_t* active, int32_t* result,
                            int32_t* route, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (M < 1 || M > VIEKF_BODY_MAX_M) return fail(VIEKF_ERR_INVALID, "need 1 <= M <= VIEKF_BODY_MAX_M body measurements");
  if (!types || !zdim || !rdim) return fail(VIEKF_ERR_INVALID, "types, zdim and rdim must not be null");
  if (!z || !R) return fail(VIEKF_ERR_INVALID, "z and R must not be null");
  if (r_mode < 0 || r_mode > 1) return fail(VIEKF_ERR_INVALID, "r_mode 0 or 1");
  unsigned long long codes = 0;
  for (int m = 0; m < M; m++) {
    const int t = types[m];
    if (!(t == VIEKF_ACC || t == VIEKF_ALT || t == VIEKF_ATT || t == VIEKF_POS || t == VIEKF_VEL))
      return fail(VIEKF_ERR_INVALID, "viekf_batch_update_body takes ACC, ALT, ATT, POS and VEL (feature models: viekf_batch_update)");
    if (zdim[m] < 1 || zdim[m] > 4 || rdim[m] < 1 || rdim[m] > 3) return fail(VIEKF_ERR_INVALID, "need 1 <= zdim <= 4, 1 <= rdim <= 3");
    codes |= body_code(t, zdim[m], rdim[m]) << (8 * m);
  }
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const BodyLds L(b->nxs, b->n, M);
  size_t limit = 0;
  if (int rc = body_lds_limit(b->device, &limit)) return rc;
  const bool fused = L.bytes() <= limit;
  // (every family's P is the column-major matrix once it is unpacked: nothing else to ask of the batch)
  if (int rc = require_P(b, fused ? PForm::Lower : PForm::Full)) return rc;
  const double *d_z = nullptr, *d_R = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t* d_res = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(z, (size_t)M * B * 4, &d_z), in(R, r_mode ? (size_t)M * B * 9 : (size_t)M * 9, &d_R),
                        in(active, (size_t)M * B, &d_act), out(result, (size_t)M * B, &d_res)))
    return rc;
  StreamArgs a = make_args(b);
  const long rsm = r_mode ? 9L * (long)B : 9L, rsb = r_mode ? 9L : 0L;
  if (fused) {
    static size_t have[64] = {};
    if (int rc = raise_dyn_lds({&k_update_body_n<kThreads>}, L.bytes(), have[b->device & 63])) return rc;
    hipLaunchKernelGGL(k_update_body_n<kThreads>, dim3(b->B), dim3(kThreads), L.bytes(), b->stream, a, M, codes, d_z, d_R, rsm, rsb,
                       d_act, d_res);
    HIP_TRY(hipGetLastError());
    b->book.wrote_live(PForm::Lower);   // (reads and writes the lower triangle only)
  } else {
    if (!b->d_body_z)
      if (int rc = b->own.alloc(&b->d_body_z, (size_t)VIEKF_BODY_MAX_M * B * 4)) return rc;
    for (int m = 0; m < M; m++) {   // entry m exactly as viekf_batch_update launches it; z in the [B][zdim] rows that kernel reads
      double* zp = b->d_body_z + (size_t)m * B * 4;
      hipLaunchKernelGGL(k_body_pack_z, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, b->stream, b->B, zdim[m], d_z + (size_t)m * B * 4, zp);
      hipLaunchKernelGGL(k_update_generic<kThreads>, dim3(b->B), dim3(kThreads), GenLds(b->nxs, b->n).bytes(), b->stream, a, types[m],
                         zdim[m], rdim[m], zp, nullptr, d_R + rsm * m, rsb, d_act ? d_act + (size_t)m * B : nullptr,
                         d_res ? d_res + (size_t)m * B : nullptr);
      HIP_TRY(hipGetLastError());
    }
  }
  if (route) *route = fused ? 1 : 0;
  return st.finish();
}

}  // extern "C"
