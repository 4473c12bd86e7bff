// viekf_capi_frame.hpp -- the device-resident frame intake (include/viekf_frame.h; its own kernels in viekf_kernels_frame.hpp):
// the handle with its feature-id tables, how the rows grow with a frame's length, and the entry points.  The intake launches
// the batch's own kernels (keep, keyframe reset, init, the FEAT update) through viekf_dispatch.hpp, which is why this is part
// of the one translation unit: included by viekf_capi.hip ONLY.
#pragma once
#include <cmath>

#include "../../include/viekf_frame.h"
#include "viekf_dispatch.hpp"
#include "viekf_kernels_frame.hpp"
#include "viekf_staging.hpp"

struct viekf_frame {
  viekf_batch* b = nullptr;
  int device = 0;
  DevOwner own;   // the tables of t
  FrameTabs t = {};
  int mcap = 0;   // capacity of the M-sized rows (grown when a frame is longer; they are addressed with the call's own M)
};

namespace {

int check_frame(const viekf_frame* f) {
  if (!f || !f->b) return fail(VIEKF_ERR_INVALID, "null frame intake handle");
  return VIEKF_OK;
}

// rows for frames of up to M entries: the per-frame arrays are simply replaced, the keyframe lists move into wider rows
int frame_reserve(viekf_frame* f, int M) {
  if (M <= f->mcap) return VIEKF_OK;
  viekf_batch* b = f->b;
  FrameTabs& t = f->t;
  const size_t B = (size_t)b->B;
  const int cap = std::max(64, std::max(M, b->N));
  DevOwner& own = f->own;
  HIP_TRY(hipStreamSynchronize(b->stream));
  // (six rows under one capacity and one synchronise: free and alloc rather than six reserves)
  int rc = own.free(&t.code);
  if (!rc) rc = own.free(&t.pos);
  if (!rc) rc = own.free(&t.slot_u);
  if (!rc) rc = own.free(&t.z_u);
  if (!rc) rc = own.free(&t.R_u);
  if (!rc) rc = own.free(&t.res_u);
  f->mcap = 0;
  if (!rc) rc = own.alloc(&t.code, B * cap);
  if (!rc) rc = own.alloc(&t.pos, B * cap);
  if (!rc) rc = own.alloc(&t.slot_u, B * cap);
  if (!rc) rc = own.alloc(&t.res_u, B * cap);
  if (!rc) rc = own.alloc(&t.z_u, 2 * B * cap);
  if (!rc) rc = own.alloc(&t.R_u, 4 * B * cap);
  int* kf = nullptr;
  if (!rc) rc = own.alloc(&kf, B * cap);
  if (rc) return rc;
  hipError_t e = hipMemset(kf, 0xff, sizeof(int) * B * cap);
  if (e == hipSuccess && t.kf)
    e = hipMemcpy2D(kf, sizeof(int) * cap, t.kf, sizeof(int) * t.kfcap, sizeof(int) * t.kfcap, B, hipMemcpyDeviceToDevice);
  if (e != hipSuccess) { (void)own.free(&kf); return fail(VIEKF_ERR_HIP, std::string("keyframe list move failed: ") + hipGetErrorString(e)); }
  if (int rc2 = own.free(&t.kf)) return rc2;
  t.kf = kf; t.kfcap = cap;
  f->mcap = cap;
  return VIEKF_OK;
}

int check_gyro_var(double gyro_var) {
  if (!(gyro_var >= 0.0) || !std::isfinite(gyro_var)) return fail(VIEKF_ERR_INVALID, "gyro_var must be finite and >= 0");
  return VIEKF_OK;
}

// What the intake's measurement steps (viekf_frame_intake_depth, viekf_frame_intake_pixel_vel) check alike, in their order and
// under the entry point's own messages, then the rows for M entries.  have_all: none of the step's arrays is null; gyro_var:
// NULL where the step has none.
struct IntakeStepMsgs { const char *m_range, *null_arg, *mask; };
int intake_step_begin(viekf_frame* f, int M, int max_M, bool have_all, int r_mode, const double* gyro_var, viekf_mem where,
                      const IntakeStepMsgs& msg) {
  if (int rc = check_frame(f)) return rc;
  if (M < 1 || M > max_M) return fail(VIEKF_ERR_INVALID, msg.m_range);
  if (!have_all) return fail(VIEKF_ERR_INVALID, msg.null_arg);
  if (r_mode < 0 || r_mode > 2) return fail(VIEKF_ERR_INVALID, "r_mode must be 0, 1 or 2");
  if (gyro_var)
    if (int rc = check_gyro_var(*gyro_var)) return rc;
  if (int rc = check_where(where)) return rc;
  if (f->b->active_on) return fail(VIEKF_ERR_INVALID, msg.mask);
  HIP_TRY(hipSetDevice(f->b->device));
  return frame_reserve(f, M);
}

// k_frame_slot_plan (id -> slot on the intake's table, which entries measure) on the batch's stream: the slots go to the
// intake's slot_u, the per-entry `active` (*act_d) to its code row -- per-frame rows, free again after the intake.
template <int ZD>
int intake_step_plan(viekf_frame* f, int M, const int32_t* d_ids, const double* d_val, const int32_t* d_fr, const uint8_t* d_act,
                     int use, unsigned char** act_d) {
  viekf_batch* b = f->b;
  const FrameTabs& t = f->t;
  *act_d = reinterpret_cast<unsigned char*>(t.code);
  hipLaunchKernelGGL(k_frame_slot_plan<ZD>, dim3(b->B), dim3(64), 0, b->stream, b->B, b->N, M, b->d_len, t.tab, t.tlen, d_ids, d_val, d_fr,
                     d_act, use ? 1 : 0, t.slot_u, *act_d);
  HIP_TRY(hipGetLastError());
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int viekf_frame_destroy(viekf_frame* f) {
  if (!f) return fail(VIEKF_ERR_INVALID, "null frame intake handle");
  (void)hipSetDevice(f->device);
  (void)hipDeviceSynchronize();   // (not the batch's stream: the tables may be freed after their batch is gone)
  f->own.release_all();
  delete f;
  return VIEKF_OK;
}

int viekf_frame_create(viekf_batch* b, viekf_frame** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  viekf_frame* f = new viekf_frame();
  f->b = b; f->device = b->device;
  FrameTabs& t = f->t;
  const size_t B = (size_t)b->B, BN = B * (size_t)b->N;
  DevOwner& own = f->own;
  int rc = own.alloc(&t.tab, BN);
  if (!rc) rc = own.alloc(&t.tlen, B);
  if (!rc) rc = own.alloc(&t.kflen, B);
  if (!rc) rc = own.alloc(&t.keep, BN);
  if (!rc) rc = own.alloc(&t.rmask, B);
  if (!rc) rc = own.alloc(&t.newcnt, B);
  if (!rc) rc = own.alloc(&t.newpix, 2 * BN);
  if (!rc) rc = own.alloc(&t.newdepth, BN);
  if (!rc) rc = frame_reserve(f, std::max(64, b->N));
  if (!rc) rc = viekf_frame_reset(f);
  if (rc) { viekf_frame_destroy(f); return rc; }
  *out = f;
  return VIEKF_OK;
}

int viekf_frame_reset(viekf_frame* f) {
  if (int rc = check_frame(f)) return rc;
  viekf_batch* b = f->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  HIP_TRY(hipMemsetAsync(f->t.tab, 0xff, sizeof(int) * std::max<size_t>(B * b->N, 1), b->stream));   // (-1)
  HIP_TRY(hipMemsetAsync(f->t.tlen, 0, sizeof(int) * B, b->stream));
  HIP_TRY(hipMemsetAsync(f->t.kflen, 0, sizeof(int) * B, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_frame_set_tracked(viekf_frame* f, const int32_t* ids, viekf_mem where) {
  if (int rc = check_frame(f)) return rc;
  if (!ids) return fail(VIEKF_ERR_INVALID, "ids is null");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = f->b;
  HIP_TRY(hipSetDevice(b->device));
  const int B = b->B, N = b->N;
  if (where == VIEKF_HOST) {   // row b: len_features[b] distinct ids >= 0, then -1
    std::vector<int32_t> len((size_t)B);
    HIP_TRY(hipMemcpyAsync(len.data(), b->d_len, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    for (int i = 0; i < B; i++) {
      const int32_t* row = ids + (size_t)i * N;
      for (int k = 0; k < N; k++) {
        if (k < len[(size_t)i] ? row[k] < 0 : row[k] != -1)
          return fail(VIEKF_ERR_INVALID, "set_tracked: a row must hold len_features ids >= 0, then -1 (wrong length)");
        for (int j = 0; k < len[(size_t)i] && j < k; j++)
          if (row[j] == row[k]) return fail(VIEKF_ERR_INVALID, "set_tracked: duplicate id in a row");
      }
    }
  }
  if (int rc = copy_user(f->t.tab, ids, sizeof(int32_t) * (size_t)B * N, where, Copy::FromUser, b->stream)) return rc;
  hipLaunchKernelGGL(k_frame_adopt, dim3(B), dim3(64), 0, b->stream, B, N, f->t.tab, f->t.tlen);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_frame_tracked(viekf_frame* f, int32_t* ids, int32_t* len, viekf_mem where) {
  if (int rc = check_frame(f)) return rc;
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = f->b;
  HIP_TRY(hipSetDevice(b->device));
  if (b->N > 0)
    if (int rc = copy_user(ids, f->t.tab, sizeof(int32_t) * (size_t)b->B * b->N, where, Copy::ToUser, b->stream)) return rc;
  if (int rc = copy_user(len, f->t.tlen, sizeof(int32_t) * (size_t)b->B, where, Copy::ToUser, b->stream)) return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

// plan -> k_keep_features -> k_keyframe_reset -> k_init_features -> the batch's FEAT update -> finish, all on the batch's
// stream and nothing of it waited for; the host never learns how many features a filter dropped or started.
int viekf_frame_intake(viekf_frame* f, int32_t M, const double* z, const int32_t* ids, const double* depth, const double* R,
                       int32_t r_mode, const uint8_t* active, int32_t* result, int32_t* gated, int32_t* gated_count,
                       uint8_t* did_reset, double* edges, viekf_mem where) {
  if (int rc = check_frame(f)) return rc;
  viekf_batch* b = f->b;
  if (M < 1 || M > VIEKF_FRAME_MAX_M) return fail(VIEKF_ERR_INVALID, "need 1 <= M <= 4096 entries per frame");
  if (!z || !ids || !R) return fail(VIEKF_ERR_INVALID, "z, ids and R must not be null");
  if (r_mode < 0 || r_mode > 2) return fail(VIEKF_ERR_INVALID, "r_mode must be 0, 1 or 2");
  if (int rc = check_where(where)) return rc;
  if (b->active_on)
    return fail(VIEKF_ERR_INVALID, "viekf_frame_intake under a participation mask (viekf_batch_set_active(NULL) first; the call takes its own `active`)");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = frame_reserve(f, M)) return rc;
  // keep and reset read and write all of P; the host cannot know whether either will have anything to do
  if (int rc = require_P(b, PForm::Full)) return rc;
  const size_t B = (size_t)b->B, BM = B * (size_t)M;
  const double *d_z = nullptr, *d_depth = nullptr, *d_R = nullptr;
  const int32_t* d_ids = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t *d_res = nullptr, *d_gated = nullptr, *d_gc = nullptr;
  uint8_t* d_dr = nullptr;
  double* d_edges = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(z, 2 * BM, &d_z), in(ids, BM, &d_ids), in(depth, BM, &d_depth), in(R, r_count(b, M, r_mode), &d_R),
                        in(active, B, &d_act), out(result, BM, &d_res), out(gated, BM, &d_gated), out(gated_count, B, &d_gc),
                        out(did_reset, B, &d_dr), out(edges, 17 * B, &d_edges)))
    return rc;
  const FrameTabs& t = f->t;
  StreamArgs a = make_args(b);
  const int use_kfr = b->params.use_keyframe_reset != 0;
  const size_t plds = sizeof(int) * (2 * (size_t)M + 2 * (size_t)b->N);
  hipLaunchKernelGGL(k_frame_plan, dim3(b->B), dim3(64), plds, b->stream, a, t, M, d_z, d_ids, d_depth, d_R, r_mode, d_act, use_kfr,
                     b->params.keyframe_overlap_threshold, d_edges);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_keep_features<kThreads>, dim3(b->B), dim3(kThreads), KeepLds(b->n).bytes(), b->stream, a, t.keep, nullptr);
  HIP_TRY(hipGetLastError());
  if (use_kfr) {
    hipLaunchKernelGGL(k_keyframe_reset<kThreads>, dim3(b->B), dim3(kThreads), 0, b->stream, a, t.rmask, d_edges);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_init_features<kThreads>, dim3(b->B), dim3(kThreads), 0, b->stream, a, t.newcnt, t.newpix, t.newdepth);
  HIP_TRY(hipGetLastError());
  const double* Ru = r_mode == 2 ? t.R_u : d_R;
  if (use_resident(b)) {
    if (int rc = launch_resident(b, false, nullptr, nullptr, t.z_u, t.slot_u, M, Ru, r_mode, t.res_u)) return rc;
  } else {
    if (int rc = launch_update(b, t.z_u, t.slot_u, M, Ru, r_mode, t.res_u)) return rc;
  }
  hipLaunchKernelGGL(k_frame_finish, dim3(b->B), dim3(64), 0, b->stream, b->B, t, M, d_ids, d_res, d_gated, d_gc, d_dr);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

}  // extern "C"
