// viekf_capi_pixvel.hpp -- the PIXEL_VEL measurement's entry points (include/viekf_pixvel.h; kernels in
// viekf_kernels_pixvel.hpp): the checks, the launches of the single-entry kernel, the read-only evaluation, the flow by id and
// the intake's pixel-velocity step.  Launches the batch's kernels through viekf_dispatch.hpp and uses the intake's handle:
// included by viekf_capi.hip ONLY, after viekf_capi_frame.hpp.
#pragma once
#include <cmath>

#include "../../include/viekf_pixvel.h"
#include "viekf_capi_body.hpp"
#include "viekf_capi_frame.hpp"
#include "viekf_dispatch.hpp"
#include "viekf_pixvel_lds.hpp"
#include "viekf_staging.hpp"

static_assert(VIEKF_PIXVELS_MAX_M == kPixvelsMaxM, "the header's limit is the kernel's");

namespace {

// The launches of viekf_batch_update_pixel_vels on device pointers (checked by the caller): the one fused launch where its
// layout fits what the device gives a workgroup (and the batch is not held to route 0), else entry by entry, in `order`.
int pixvels_launch(viekf_batch* b, int M, const int32_t* d_slot, const double* d_z, const double* d_gyro, const double* d_R, int r_mode,
                   double gyro_var, const uint8_t* d_act, int order, int32_t* d_res, int32_t* route) {
  const PixvelLds L(b->nxs, b->n);
  size_t limit = 0;
  if (int rc = body_lds_limit(b->device, &limit)) return rc;
  const PixvelsLds LF(b->nxs, b->n, b->N, M);
  if (b->pixvel_route != 0 && LF.bytes() <= limit) {
    if (int rc = require_P(b, PForm::Lower)) return rc;
    static size_t have_f[64] = {};
    if (int rc = raise_dyn_lds({&k_update_pixvels<kThreads>}, LF.bytes(), have_f[b->device & 63])) return rc;
    StreamArgs a = make_args(b);
    long rsb = 0, rsm = 0;
    r_strides(r_mode, M, &rsb, &rsm);
    hipLaunchKernelGGL(k_update_pixvels<kThreads>, dim3(b->B), dim3(kThreads), LF.bytes(), b->stream, a, M, order, d_slot, d_z, d_gyro, d_R,
                       rsb, rsm, gyro_var, d_act, d_res);
    HIP_TRY(hipGetLastError());
    b->book.wrote_live(PForm::Lower);   // (reads and writes the lower triangle only)
    if (route) *route = 1;
    return VIEKF_OK;
  }
  if (L.bytes() > limit) return fail(VIEKF_ERR_UNSUPPORTED, "num_features too large for the PIXEL_VEL update's LDS layout");
  if (int rc = require_P(b, PForm::Full)) return rc;   // (the kernel reads whole columns)
  static size_t have[64] = {};
  if (int rc = raise_dyn_lds({&k_update_pixvel<kThreads>}, L.bytes(), have[b->device & 63])) return rc;
  StreamArgs a = make_args(b);
  long rsb = 0, rsm = 0;
  r_strides(r_mode, M, &rsb, &rsm);
  for (int e = 0; e < M; e++) {
    const int m = order ? M - 1 - e : e;
    hipLaunchKernelGGL(k_update_pixvel<kThreads>, dim3(b->B), dim3(kThreads), L.bytes(), b->stream, a, M, m, d_slot, d_z, d_gyro, d_R, rsb,
                       rsm, gyro_var, d_act, d_res);
    HIP_TRY(hipGetLastError());
  }
  if (route) *route = 0;
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int64_t viekf_pixvels_lds_bytes(int32_t num_features, int32_t M) {
  int nxs = 0, n = 0;
  if (!lds_dims(num_features, &nxs, &n) || M < 1 || M > VIEKF_PIXVELS_MAX_M) return 0;
  return (int64_t)PixvelsLds(nxs, n, num_features, M).bytes();
}

int viekf_batch_pixel_vels_route(viekf_batch* b, int32_t route) {
  if (int rc = check_batch(b)) return rc;
  if (route < -1 || route > 1) return fail(VIEKF_ERR_INVALID, "route must be -1 (automatic), 0 or 1");
  b->pixvel_route = route;
  return VIEKF_OK;
}

int64_t viekf_pixvel_lds_bytes(int32_t num_features) {
  int nxs = 0, n = 0;
  return lds_dims(num_features, &nxs, &n) ? (int64_t)PixvelLds(nxs, n).bytes() : 0;
}

int viekf_batch_update_pixel_vels(viekf_batch* b, int32_t M, const int32_t* slot, const double* z, const double* gyro, const double* R,
                                  int32_t r_mode, double gyro_var, const uint8_t* active, int32_t order, int32_t* result,
                                  int32_t* route, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (M < 1 || M > VIEKF_PIXVELS_MAX_M) return fail(VIEKF_ERR_INVALID, "need 1 <= M <= VIEKF_PIXVELS_MAX_M pixel-velocity measurements");
  if (!slot || !z || !gyro || !R) return fail(VIEKF_ERR_INVALID, "slot, z, gyro and R must not be null");
  if (r_mode < 0 || r_mode > 2) return fail(VIEKF_ERR_INVALID, "r_mode must be 0, 1 or 2");
  if (order != 0 && order != 1) return fail(VIEKF_ERR_INVALID, "order must be 0 or 1");
  if (int rc = check_gyro_var(gyro_var)) return rc;
  if (int rc = check_where(where)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B, BM = B * (size_t)M;
  const int32_t* d_slot = nullptr;
  const double *d_z = nullptr, *d_g = nullptr, *d_R = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t* d_res = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(slot, BM, &d_slot), in(z, 2 * BM, &d_z), in(gyro, 3 * B, &d_g), in(R, r_count(b, M, r_mode), &d_R),
                        in(active, BM, &d_act), out(result, BM, &d_res)))
    return rc;
  if (int rc = pixvels_launch(b, M, d_slot, d_z, d_g, d_R, r_mode, gyro_var, d_act, order, d_res, route)) return rc;
  return st.finish();
}

int viekf_batch_eval_pixel_vel(viekf_batch* b, const int32_t* slot, const double* gyro, double* zhat, double* H, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!slot || !gyro || !zhat) return fail(VIEKF_ERR_INVALID, "slot, gyro and zhat must not be null");
  if (int rc = check_where(where)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const int32_t* d_slot = nullptr;
  const double* d_g = nullptr;
  double *d_z = nullptr, *d_H = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(slot, B, &d_slot), in(gyro, 3 * B, &d_g), out(zhat, 2 * B, &d_z), out(H, 2 * B * b->n, &d_H))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_eval_pixel_vel, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, a, d_slot, d_g, d_z, d_H);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_pixel_flow(viekf_batch* b, int32_t M_prev, const double* z_prev, const int32_t* ids_prev, int32_t M, const double* z,
                     const int32_t* ids, const double* dt, double* zdot, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (M < 1 || M > VIEKF_PIXEL_FLOW_MAX_M || M_prev < 1 || M_prev > VIEKF_PIXEL_FLOW_MAX_M)
    return fail(VIEKF_ERR_INVALID, "need 1 <= M_prev, M <= VIEKF_PIXEL_FLOW_MAX_M");
  if (!z_prev || !ids_prev || !z || !ids || !dt || !zdot) return fail(VIEKF_ERR_INVALID, "viekf_pixel_flow: null argument");
  if (int rc = check_where(where)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const double *d_zp = nullptr, *d_z = nullptr, *d_dt = nullptr;
  const int32_t *d_ip = nullptr, *d_i = nullptr;
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(z_prev, 2 * B * M_prev, &d_zp), in(ids_prev, B * M_prev, &d_ip), in(z, 2 * B * M, &d_z), in(ids, B * M, &d_i),
                        in(dt, B, &d_dt), out(zdot, 2 * B * M, &d_o)))
    return rc;
  hipLaunchKernelGGL(k_pixel_flow, dim3(b->B), dim3(64), 0, b->stream, b->B, M_prev, d_zp, d_ip, M, d_z, d_i, d_dt, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

// intake_step_plan -> the update's launches, all on the batch's stream.
int viekf_frame_intake_pixel_vel(viekf_frame* f, int32_t M, const int32_t* ids, const double* zdot, const int32_t* feat_result,
                                 const double* gyro, const double* R, int32_t r_mode, double gyro_var, int32_t use_pixel_vel,
                                 const uint8_t* active, int32_t* result, viekf_mem where) {
  static const IntakeStepMsgs msg = {
      "need 1 <= M <= VIEKF_PIXVELS_MAX_M entries per frame", "ids, zdot, feat_result, gyro and R must not be null",
      "viekf_frame_intake_pixel_vel under a participation mask (viekf_batch_set_active(NULL) first; the call takes its own `active`)"};
  if (int rc = intake_step_begin(f, M, VIEKF_PIXVELS_MAX_M, ids && zdot && feat_result && gyro && R, r_mode, &gyro_var, where, msg))
    return rc;
  viekf_batch* b = f->b;
  const size_t B = (size_t)b->B, BM = B * (size_t)M;
  const int32_t *d_ids = nullptr, *d_fr = nullptr;
  const double *d_zd = nullptr, *d_g = nullptr, *d_R = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t* d_res = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(ids, BM, &d_ids), in(zdot, 2 * BM, &d_zd), in(feat_result, BM, &d_fr), in(gyro, 3 * B, &d_g),
                        in(R, r_count(b, M, r_mode), &d_R), in(active, B, &d_act), out(result, BM, &d_res)))
    return rc;
  unsigned char* act_d = nullptr;
  if (int rc = intake_step_plan<2>(f, M, d_ids, d_zd, d_fr, d_act, use_pixel_vel, &act_d)) return rc;
  if (int rc = pixvels_launch(b, M, f->t.slot_u, d_zd, d_g, d_R, r_mode, gyro_var, act_d, 1, d_res, nullptr)) return rc;
  return st.finish();
}

}  // extern "C"
