// viekf_capi_map.hpp -- the device-resident landmark map (include/viekf_map.h; kernels in viekf_kernels_map.hpp): the handle
// with its store, and the entry points.  It reads the batch's book (the form of P), the frame intake's id table and the node
// graph's nodes: included by viekf_capi.hip ONLY, after viekf_capi_frame.hpp and viekf_capi_node.hpp.
#pragma once
#include "../../include/viekf_map.h"
#include "viekf_dispatch.hpp"
#include "viekf_kernels_map.hpp"
#include "viekf_staging.hpp"

struct viekf_map {
  viekf_batch* b = nullptr;
  viekf_frame* f = nullptr;   // or null: no store, no error
  viekf_node* nd = nullptr;   // or null: identity nodes
  int device = 0;
  DevOwner own;   // the tables of t
  MapTabs t = {};
};

namespace {

int check_map(const viekf_map* m) {
  if (!m || !m->b) return fail(VIEKF_ERR_INVALID, "null landmark map handle");
  return VIEKF_OK;
}

// a lane per feature slot: one, two or four waves (viekf_kernels_map.hpp loops past that)
unsigned map_block(const viekf_batch* b) { return b->N <= 64 ? 64u : (b->N <= 128 ? 128u : (unsigned)MP_MAX_T); }

const double* map_node(const viekf_map* m) { return m->nd ? m->nd->t.node : nullptr; }

}  // namespace

extern "C" {

int viekf_map_destroy(viekf_map* m) {
  if (!m) return fail(VIEKF_ERR_INVALID, "null landmark map handle");
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();   // (not the batch's stream: the tables may be freed after their batch is gone)
  m->own.release_all();
  delete m;
  return VIEKF_OK;
}

int viekf_map_create(viekf_batch* b, viekf_frame* frame, viekf_node* node, int32_t capacity, viekf_map** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_batch(b)) return rc;
  if (capacity < 0 || capacity > VIEKF_MAP_MAX_CAPACITY) return fail(VIEKF_ERR_INVALID, "need 0 <= capacity <= 4096");
  if (frame && frame->b != b) return fail(VIEKF_ERR_INVALID, "the frame intake belongs to another batch");
  if (node && node->b != b) return fail(VIEKF_ERR_INVALID, "the node graph belongs to another batch");
  if (capacity > 0 && !frame) return fail(VIEKF_ERR_INVALID, "a store (capacity > 0) needs the frame intake: it is keyed by the intake's ids");
  HIP_TRY(hipSetDevice(b->device));
  viekf_map* m = new viekf_map();
  m->b = b; m->f = frame; m->nd = node; m->device = b->device;
  MapTabs& t = m->t;
  t.cap = capacity;
  const size_t rows = (size_t)b->B * (size_t)capacity;
  DevOwner& own = m->own;
  int rc = own.alloc(&t.id, rows);
  if (!rc) rc = own.alloc(&t.pos, 3 * rows);
  if (!rc) rc = own.alloc(&t.cov, 6 * rows);
  if (!rc) rc = own.alloc(&t.nobs, rows);
  if (!rc) rc = own.alloc(&t.ncount, rows);
  if (!rc) rc = viekf_map_reset(m);
  if (rc) { viekf_map_destroy(m); return rc; }
  *out = m;
  return VIEKF_OK;
}

int viekf_map_reset(viekf_map* m) {
  if (int rc = check_map(m)) return rc;
  viekf_batch* b = m->b;
  HIP_TRY(hipSetDevice(b->device));
  const MapTabs& t = m->t;
  const size_t rows = (size_t)b->B * (size_t)t.cap;
  if (rows) {
    HIP_TRY(hipMemsetAsync(t.id, 0xff, sizeof(int) * rows, b->stream));   // (-1)
    HIP_TRY(hipMemsetAsync(t.pos, 0, sizeof(double) * 3 * rows, b->stream));
    HIP_TRY(hipMemsetAsync(t.cov, 0, sizeof(double) * 6 * rows, b->stream));
    HIP_TRY(hipMemsetAsync(t.nobs, 0, sizeof(int) * rows, b->stream));
    HIP_TRY(hipMemsetAsync(t.ncount, 0, sizeof(int) * rows, b->stream));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

// read-only; a packed P goes to the canonical lower form first (the feature diagonal blocks of the packed image live behind the
// ownership map), as viekf_diag_consistency has it
int viekf_map_landmarks(viekf_map* m, double* pos_node, double* cov_node, double* pos_global, double* cov_global, viekf_mem where) {
  if (int rc = check_map(m)) return rc;
  if (!pos_node && !cov_node && !pos_global && !cov_global) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = m->b;
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;
  const size_t BN = (size_t)b->B * (size_t)b->N;
  double *d_pn = nullptr, *d_cn = nullptr, *d_pg = nullptr, *d_cg = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(out(pos_node, 3 * BN, &d_pn), out(cov_node, 6 * BN, &d_cn), out(pos_global, 3 * BN, &d_pg), out(cov_global, 6 * BN, &d_cg)))
    return rc;
  hipLaunchKernelGGL(k_map_landmarks, dim3(b->B), dim3(map_block(b)), 0, b->stream, make_args(b), map_node(m), d_pn, d_cn, d_pg, d_cg);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_map_update(viekf_map* m) {
  if (int rc = check_map(m)) return rc;
  if (m->t.cap == 0) return VIEKF_OK;
  viekf_batch* b = m->b;
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;
  const size_t lds = sizeof(int) * (size_t)std::max(b->N, 1);
  hipLaunchKernelGGL(k_map_update, dim3(b->B), dim3(map_block(b)), lds, b->stream, make_args(b), m->f->t.tab, m->f->t.tlen, map_node(m),
                     m->nd ? m->nd->t.count : nullptr, m->t);
  HIP_TRY(hipGetLastError());
  return VIEKF_OK;
}

static int map_copy(viekf_map* m, bool get, void* ids, void* pos, void* cov, void* n_obs, void* node_count, viekf_mem where) {
  if (int rc = check_map(m)) return rc;
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = m->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t rows = (size_t)b->B * (size_t)m->t.cap;
  const MapTabs& t = m->t;
  struct Arr { void* user; void* dev; size_t bytes; } arrs[] = {{ids, t.id, sizeof(int32_t) * rows}, {pos, t.pos, sizeof(double) * 3 * rows},
                                                                {cov, t.cov, sizeof(double) * 6 * rows}, {n_obs, t.nobs, sizeof(int32_t) * rows},
                                                                {node_count, t.ncount, sizeof(int32_t) * rows}};
  if (rows)
    for (const Arr& a : arrs)
      if (int rc = copy_user(get ? a.user : a.dev, get ? a.dev : a.user, a.bytes, where, get ? Copy::ToUser : Copy::FromUser, b->stream)) return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_map_get(viekf_map* m, int32_t* ids, double* pos, double* cov, int32_t* n_obs, int32_t* node_count, viekf_mem where) {
  return map_copy(m, true, ids, pos, cov, n_obs, node_count, where);
}

int viekf_map_set(viekf_map* m, const int32_t* ids, const double* pos, const double* cov, const int32_t* n_obs, const int32_t* node_count,
                  viekf_mem where) {
  return map_copy(m, false, const_cast<int32_t*>(ids), const_cast<double*>(pos), const_cast<double*>(cov), const_cast<int32_t*>(n_obs),
                  const_cast<int32_t*>(node_count), where);
}

int viekf_map_error(viekf_map* m, const double* lm_true, int32_t per_vehicle, int32_t L, const int32_t* frame_ids, const int32_t* landmark,
                    int32_t M, double* err_node, double* nees, int32_t* info, double* err_global, viekf_mem where) {
  if (int rc = check_map(m)) return rc;
  if (!m->f) return fail(VIEKF_ERR_INVALID, "viekf_map_error needs the frame intake (viekf_map_create was given none)");
  if (!lm_true || !frame_ids || !landmark) return fail(VIEKF_ERR_INVALID, "lm_true, frame_ids and landmark must not be null");
  if (!err_node && !nees && !info && !err_global) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (L < 1) return fail(VIEKF_ERR_INVALID, "need L >= 1 landmarks");
  if (M < 1 || M > VIEKF_FRAME_MAX_M) return fail(VIEKF_ERR_INVALID, "need 1 <= M <= 4096 entries per frame");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = m->b;
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;
  const size_t B = (size_t)b->B, BN = B * (size_t)b->N, BM = B * (size_t)M;
  const double* d_lm = nullptr;
  const int32_t *d_fid = nullptr, *d_flm = nullptr;
  double *d_en = nullptr, *d_ne = nullptr, *d_eg = nullptr;
  int32_t* d_info = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(lm_true, 3 * (size_t)L * (per_vehicle ? B : 1), &d_lm), in(frame_ids, BM, &d_fid), in(landmark, BM, &d_flm),
                        out(err_node, 3 * BN, &d_en), out(nees, BN, &d_ne), out(info, BN, &d_info), out(err_global, 3 * BN, &d_eg)))
    return rc;
  const size_t lds = sizeof(int) * 2 * (size_t)M;
  hipLaunchKernelGGL(k_map_error, dim3(b->B), dim3(map_block(b)), lds, b->stream, make_args(b), m->f->t.tab, m->f->t.tlen, map_node(m),
                     m->nd ? m->nd->t.tnode : nullptr, d_lm, per_vehicle != 0, L, d_fid, d_flm, M, d_en, d_ne, d_info, d_eg);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

}  // extern "C"
