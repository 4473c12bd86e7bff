// viekf_capi_rec.hpp -- the device-resident flight recorder (include/viekf_rec.h; kernels in viekf_kernels_rec.hpp): the handle
// with its tables, the frame counter and the stamps on the host, and the entry points.  It uses the batch's size, device and
// stream only: included by viekf_capi.hip ONLY, after viekf_capi_map.hpp.
#pragma once
#include "../../include/viekf_rec.h"
#include "viekf_dispatch.hpp"
#include "viekf_kernels_rec.hpp"
#include "viekf_staging.hpp"

struct viekf_rec {
  viekf_batch* b = nullptr;
  int device = 0;
  DevOwner own;                 // the tables of t, and res / res_n
  RecTabs t = {};
  int count = 0;                // frames held: the one frame index of the whole recorder
  std::vector<double> stamps;   // [count]
  double* res = nullptr;        // [B][11]: the trajectory error's double outputs on their way to a host caller
  int* res_n = nullptr;         // [B][2]
};

namespace {

int check_rec(const viekf_rec* r) {
  if (!r || !r->b) return fail(VIEKF_ERR_INVALID, "null flight recorder handle");
  return VIEKF_OK;
}

// first <= k < last inside the frames held; last = -1 is count
int rec_range(const viekf_rec* r, int32_t first, int32_t* last) {
  if (*last == -1) *last = r->count;
  if (first < 0 || *last < first || *last > r->count) return fail(VIEKF_ERR_INVALID, "need 0 <= first <= last <= count (last = -1: count)");
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int viekf_rec_destroy(viekf_rec* r) {
  if (!r) return fail(VIEKF_ERR_INVALID, "null flight recorder handle");
  (void)hipSetDevice(r->device);
  (void)hipDeviceSynchronize();   // (not the batch's stream: the tables may be freed after their batch is gone)
  r->own.release_all();
  delete r;
  return VIEKF_OK;
}

int viekf_rec_create(viekf_batch* b, int32_t capacity, int32_t channels, viekf_rec** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_batch(b)) return rc;
  if (capacity < 1 || capacity > VIEKF_REC_MAX_FRAMES) return fail(VIEKF_ERR_INVALID, "need 1 <= capacity <= 4096 frames");
  if (channels < 0 || channels > VIEKF_REC_MAX_CHANNELS) return fail(VIEKF_ERR_INVALID, "need 0 <= channels <= 8");
  HIP_TRY(hipSetDevice(b->device));
  viekf_rec* r = new viekf_rec();
  r->b = b; r->device = b->device;
  RecTabs& t = r->t;
  t.cap = capacity; t.K = channels;
  const size_t B = (size_t)b->B, rows = B * (size_t)capacity;
  DevOwner& own = r->own;
  int rc = own.alloc(&t.est, 7 * rows);
  if (!rc) rc = own.alloc(&t.tru, 7 * rows);
  if (!rc) rc = own.alloc(&t.valid, rows);
  if (!rc) rc = own.alloc(&t.chan, rows * (size_t)channels);
  if (!rc) rc = own.alloc(&r->res, 11 * B);
  if (!rc) rc = own.alloc(&r->res_n, 2 * B);
  if (rc) { viekf_rec_destroy(r); return rc; }
  r->stamps.reserve((size_t)capacity);
  *out = r;
  return VIEKF_OK;
}

int viekf_rec_reset(viekf_rec* r) {
  if (int rc = check_rec(r)) return rc;
  r->count = 0;
  r->stamps.clear();
  return VIEKF_OK;
}

int viekf_rec_count(const viekf_rec* r, int32_t* count) {
  if (int rc = check_rec(r)) return rc;
  if (!count) return fail(VIEKF_ERR_INVALID, "count is null");
  *count = r->count;
  return VIEKF_OK;
}

int viekf_rec_push(viekf_rec* r, double stamp, const double* est_pose, const double* x_true, int32_t ldx, const double* chan,
                   const uint8_t* mask, viekf_mem where) {
  if (int rc = check_rec(r)) return rc;
  if (!est_pose || !x_true) return fail(VIEKF_ERR_INVALID, "est_pose and x_true must not be null");
  if (ldx < 10) return fail(VIEKF_ERR_INVALID, "need ldx >= 10 (position 0:3, attitude 6:10)");
  if (chan && r->t.K == 0) return fail(VIEKF_ERR_INVALID, "chan given to a recorder without channels");
  if (!chan && r->t.K > 0) return fail(VIEKF_ERR_INVALID, "chan must not be null: the recorder has channels");
  if (int rc = check_where(where)) return rc;
  if (r->count >= r->t.cap) return fail(VIEKF_ERR_INVALID, "the recorder is full (count == capacity)");
  viekf_batch* b = r->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const double *d_est = nullptr, *d_xt = nullptr, *d_ch = nullptr;
  const uint8_t* d_mask = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(est_pose, 7 * B, &d_est), in(x_true, B * (size_t)ldx, &d_xt), in(chan, B * (size_t)r->t.K, &d_ch), in(mask, B, &d_mask)))
    return rc;
  hipLaunchKernelGGL(k_rec_push, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, b->B, r->t, r->count, d_est, d_xt, ldx, d_ch, d_mask);
  HIP_TRY(hipGetLastError());
  if (int rc = st.finish()) return rc;
  r->stamps.push_back(stamp);
  r->count++;
  return VIEKF_OK;
}

// the storage is [B][capacity][..] and [capacity][B][K]; a caller gets [B][T][..] and [T][B][K] with T = count
int viekf_rec_get(viekf_rec* r, double* est, double* tru, uint8_t* valid, double* chan, double* stamps, viekf_mem where) {
  if (int rc = check_rec(r)) return rc;
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = r->b;
  HIP_TRY(hipSetDevice(b->device));
  const RecTabs& t = r->t;
  const size_t B = (size_t)b->B, T = (size_t)r->count;
  if (T == 0) return VIEKF_OK;
  const hipMemcpyKind kind = where == VIEKF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t row = 7 * sizeof(double);
  if (est) HIP_TRY(hipMemcpy2DAsync(est, T * row, t.est, (size_t)t.cap * row, T * row, B, kind, b->stream));
  if (tru) HIP_TRY(hipMemcpy2DAsync(tru, T * row, t.tru, (size_t)t.cap * row, T * row, B, kind, b->stream));
  if (valid) HIP_TRY(hipMemcpy2DAsync(valid, T, t.valid, (size_t)t.cap, T, B, kind, b->stream));
  if (t.K > 0)
    if (int rc = copy_user(chan, t.chan, sizeof(double) * T * B * (size_t)t.K, where, Copy::ToUser, b->stream)) return rc;
  if (stamps) {
    if (where == VIEKF_HOST) std::memcpy(stamps, r->stamps.data(), sizeof(double) * T);
    else HIP_TRY(hipMemcpyAsync(stamps, r->stamps.data(), sizeof(double) * T, hipMemcpyHostToDevice, b->stream));
  }
  // (a device caller's stamps come from pageable host memory that the next push may move: waited for here)
  if (where == VIEKF_HOST || stamps) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_rec_trajectory_error(viekf_rec* r, int32_t align, int32_t first, int32_t last, int32_t delta, double* ate_pos, double* ate_att,
                               double* rpe_pos, double* rpe_att, double* align_pose, int32_t* n_used, viekf_mem where) {
  if (int rc = check_rec(r)) return rc;
  if (align < 0 || align > 2) return fail(VIEKF_ERR_INVALID, "align must be 0 (none), 1 (yaw and translation) or 2 (SE(3))");
  if (delta < 1) return fail(VIEKF_ERR_INVALID, "need delta >= 1");
  if (!ate_pos && !ate_att && !rpe_pos && !rpe_att && !align_pose && !n_used) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (int rc = check_where(where)) return rc;
  if (int rc = rec_range(r, first, &last)) return rc;
  viekf_batch* b = r->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  // six outputs: a host caller's go through the recorder's own result rows (one layout for both kinds of caller: the kernel
  // does not know which it serves)
  struct Arr { double* user; double* dev; size_t count; } arrs[] = {{ate_pos, r->res, B}, {ate_att, r->res + B, B}, {rpe_pos, r->res + 2 * B, B},
                                                                       {rpe_att, r->res + 3 * B, B}, {align_pose, r->res + 4 * B, 7 * B}};
  const bool host = where == VIEKF_HOST;
  double* d[5];
  for (int i = 0; i < 5; i++) d[i] = !arrs[i].user ? nullptr : (host ? arrs[i].dev : arrs[i].user);
  int* d_n = !n_used ? nullptr : (host ? r->res_n : n_used);
  hipLaunchKernelGGL(k_rec_trajectory, dim3(b->B), dim3(kRecThreads), 0, b->stream, r->t, align, first, last, delta, d[0], d[1], d[2], d[3], d[4], d_n);
  HIP_TRY(hipGetLastError());
  if (host) {
    for (const Arr& a : arrs)
      if (int rc = copy_user(a.user, a.dev, sizeof(double) * a.count, where, Copy::ToUser, b->stream)) return rc;
    if (int rc = copy_user(n_used, r->res_n, sizeof(int32_t) * 2 * B, where, Copy::ToUser, b->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  return VIEKF_OK;
}

int viekf_rec_pose_ensemble(viekf_rec* r, int32_t first, int32_t last, double* out_, viekf_mem where) {
  if (int rc = check_rec(r)) return rc;
  if (!out_) return fail(VIEKF_ERR_INVALID, "out must not be null");
  if (int rc = check_where(where)) return rc;
  if (int rc = rec_range(r, first, &last)) return rc;
  if (last == first) return VIEKF_OK;
  viekf_batch* b = r->b;
  HIP_TRY(hipSetDevice(b->device));
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(out(out_, 4 * (size_t)(last - first), &d_o))) return rc;
  hipLaunchKernelGGL(k_rec_pose_ensemble, dim3(last - first), dim3(kRecThreads), 0, b->stream, b->B, r->t, first, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_rec_channels(viekf_rec* r, int32_t first, int32_t last, const double* lo, const double* hi, double* per_frame, double* per_filter,
                       viekf_mem where) {
  if (int rc = check_rec(r)) return rc;
  if (r->t.K == 0) return fail(VIEKF_ERR_INVALID, "the recorder has no channels");
  if (!per_frame && !per_filter) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (int rc = check_where(where)) return rc;
  if (int rc = rec_range(r, first, &last)) return rc;
  viekf_batch* b = r->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t K = (size_t)r->t.K, Tn = (size_t)(last - first);
  const double *d_lo = nullptr, *d_hi = nullptr;
  double *d_pf = nullptr, *d_pb = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(lo, K, &d_lo), in(hi, K, &d_hi), out(Tn ? per_frame : nullptr, 5 * K * Tn, &d_pf), out(per_filter, 5 * K * (size_t)b->B, &d_pb)))
    return rc;
  if (d_pf) {
    hipLaunchKernelGGL(k_rec_channels_frame, dim3(last - first), dim3(kRecThreads), 0, b->stream, b->B, r->t, first, d_lo, d_hi, d_pf);
    HIP_TRY(hipGetLastError());
  }
  if (d_pb) {
    hipLaunchKernelGGL(k_rec_channels_filter, dim3((b->B + 63) / 64, r->t.K), dim3(64), 0, b->stream, b->B, r->t, first, last, d_lo, d_hi, d_pb);
    HIP_TRY(hipGetLastError());
  }
  return st.finish();
}

}  // extern "C"
