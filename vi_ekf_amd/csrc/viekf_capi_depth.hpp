// viekf_capi_depth.hpp -- a frame's DEPTH updates in one launch (include/viekf_depth.h; kernels in viekf_kernels_depth.hpp) and
// the intake's depth step (viekf_frame_intake_depth, include/viekf_frame.h): the checks, the choice between the one fused
// launch and the M launches of k_update_generic, and the entry points.  Launches the batch's kernels through
// viekf_dispatch.hpp and uses the intake's handle: included by viekf_capi.hip ONLY, after viekf_capi_frame.hpp.
#pragma once
#include <cmath>

#include "../../include/viekf_depth.h"
#include "viekf_capi_body.hpp"
#include "viekf_capi_frame.hpp"
#include "viekf_depth_lds.hpp"
#include "viekf_dispatch.hpp"
#include "viekf_staging.hpp"

static_assert(VIEKF_DEPTHS_MAX_M == kDepthsMaxM, "the header's limit is the kernel's");

namespace {

// The launches of viekf_batch_update_depths on device pointers (checked by the caller): fused where the layout fits.
int depths_launch(viekf_batch* b, int type, int M, const int32_t* d_slot, const double* d_z, const double* d_R, int r_mode,
                  const uint8_t* d_act, int order, int32_t* d_res, int32_t* route) {
  const size_t B = (size_t)b->B;
  const DepthLds L(b->nxs, b->n, M);
  size_t limit = 0;
  if (int rc = body_lds_limit(b->device, &limit)) return rc;
  const bool fused = L.bytes() <= limit;
  if (int rc = require_P(b, fused ? PForm::Lower : PForm::Full)) return rc;
  StreamArgs a = make_args(b);
  if (fused) {
    long rsb = 0, rsm = 0;
    r_strides(r_mode, M, &rsb, &rsm, 1);
    static size_t have[64] = {};
    if (int rc = raise_dyn_lds({&k_update_depths<kThreads, MT_DEPTH>, &k_update_depths<kThreads, MT_INV_DEPTH>}, L.bytes(),
                               have[b->device & 63]))
      return rc;
    if (type == VIEKF_DEPTH)
      hipLaunchKernelGGL((k_update_depths<kThreads, MT_DEPTH>), dim3(b->B), dim3(kThreads), L.bytes(), b->stream, a, M, order, d_slot,
                         d_z, d_R, rsb, rsm, d_act, d_res);
    else
      hipLaunchKernelGGL((k_update_depths<kThreads, MT_INV_DEPTH>), dim3(b->B), dim3(kThreads), L.bytes(), b->stream, a, M, order,
                         d_slot, d_z, d_R, rsb, rsm, d_act, d_res);
    HIP_TRY(hipGetLastError());
    b->book.wrote_live(PForm::Lower);   // (reads and writes the lower triangle only)
  } else {
    if (!b->d_depth_m)
      if (int rc = b->own.alloc(&b->d_depth_m, 4 * B + 8)) return rc;
    double* z_m = b->d_depth_m;
    double* R_m = z_m + B;
    int* slot_m = reinterpret_cast<int*>(R_m + B);
    int* res_m = slot_m + B;
    unsigned char* act_m = reinterpret_cast<unsigned char*>(res_m + B);
    const unsigned grid = (unsigned)((B + 255) / 256);
    for (int e = 0; e < M; e++) {   // entry m exactly as viekf_batch_update launches it, in rows of one value per filter
      const int m = order ? M - 1 - e : e;
      hipLaunchKernelGGL(k_depths_gather, dim3(grid), dim3(256), 0, b->stream, b->B, M, m, d_slot, d_z, r_mode == 2 ? d_R : nullptr,
                         d_act, slot_m, z_m, R_m, act_m);
      hipLaunchKernelGGL(k_update_generic<kThreads>, dim3(b->B), dim3(kThreads), GenLds(b->nxs, b->n).bytes(), b->stream, a, type, 1, 1,
                         z_m, slot_m, r_mode == 2 ? R_m : d_R, r_mode == 0 ? 0L : 1L, act_m, d_res ? res_m : nullptr);
      if (d_res) hipLaunchKernelGGL(k_depths_scatter, dim3(grid), dim3(256), 0, b->stream, b->B, M, m, res_m, d_res);
      HIP_TRY(hipGetLastError());
    }
  }
  if (route) *route = fused ? 1 : 0;
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int64_t viekf_depths_lds_bytes(int32_t num_features, int32_t M) {
  int nxs = 0, n = 0;
  if (!lds_dims(num_features, &nxs, &n) || M < 1 || M > VIEKF_DEPTHS_MAX_M) return 0;
  return (int64_t)DepthLds(nxs, n, M).bytes();
}

int viekf_batch_update_depths(viekf_batch* b, int32_t type, int32_t M, const int32_t* slot, const double* z, const double* R,
                              int32_t r_mode, const uint8_t* active, int32_t order, int32_t* result, int32_t* route,
                              viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (type != VIEKF_DEPTH && type != VIEKF_INV_DEPTH)
    return fail(VIEKF_ERR_INVALID, "viekf_batch_update_depths takes VIEKF_DEPTH or VIEKF_INV_DEPTH (other models: viekf_batch_update)");
  if (M < 1 || M > VIEKF_DEPTHS_MAX_M) return fail(VIEKF_ERR_INVALID, "need 1 <= M <= VIEKF_DEPTHS_MAX_M depth measurements");
  if (!slot || !z || !R) return fail(VIEKF_ERR_INVALID, "slot, z and R must not be null");
  if (r_mode < 0 || r_mode > 2) return fail(VIEKF_ERR_INVALID, "r_mode must be 0, 1 or 2");
  if (order != 0 && order != 1) return fail(VIEKF_ERR_INVALID, "order must be 0 or 1");
  if (int rc = check_where(where)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B, BM = B * (size_t)M;
  const int32_t* d_slot = nullptr;
  const double *d_z = nullptr, *d_R = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t* d_res = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(slot, BM, &d_slot), in(z, BM, &d_z), in(R, r_count(b, M, r_mode, 1), &d_R), in(active, BM, &d_act),
                        out(result, BM, &d_res)))
    return rc;
  if (int rc = depths_launch(b, type, M, d_slot, d_z, d_R, r_mode, d_act, order, d_res, route)) return rc;
  return st.finish();
}

// intake_step_plan -> viekf_batch_update_depths' launches, all on the batch's stream.
int viekf_frame_intake_depth(viekf_frame* f, int32_t M, const int32_t* ids, const double* depth, const int32_t* feat_result,
                             const double* R, int32_t r_mode, int32_t use_depth, const uint8_t* active, int32_t* result,
                             viekf_mem where) {
  static const IntakeStepMsgs msg = {
      "need 1 <= M <= VIEKF_DEPTHS_MAX_M entries per frame", "ids, depth, feat_result and R must not be null",
      "viekf_frame_intake_depth under a participation mask (viekf_batch_set_active(NULL) first; the call takes its own `active`)"};
  if (int rc = intake_step_begin(f, M, VIEKF_DEPTHS_MAX_M, ids && depth && feat_result && R, r_mode, nullptr, where, msg))
    return rc;
  viekf_batch* b = f->b;
  const size_t B = (size_t)b->B, BM = B * (size_t)M;
  const int32_t *d_ids = nullptr, *d_fr = nullptr;
  const double *d_depth = nullptr, *d_R = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t* d_res = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(ids, BM, &d_ids), in(depth, BM, &d_depth), in(feat_result, BM, &d_fr), in(R, r_count(b, M, r_mode, 1), &d_R),
                        in(active, B, &d_act), out(result, BM, &d_res)))
    return rc;
  unsigned char* act_d = nullptr;
  if (int rc = intake_step_plan<1>(f, M, d_ids, d_depth, d_fr, d_act, use_depth, &act_d)) return rc;
  if (int rc = depths_launch(b, VIEKF_DEPTH, M, f->t.slot_u, d_depth, d_R, r_mode, act_d, 1, d_res, nullptr)) return rc;
  return st.finish();
}

}  // extern "C"
