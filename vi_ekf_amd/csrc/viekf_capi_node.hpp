// viekf_capi_node.hpp -- the device-resident node graph (include/viekf_node.h; kernels in viekf_kernels_node.hpp): the handle
// with its node tables and trail, where the 21 elements of P it reads lie in whichever form P is in, and the entry points.
// It reads the batch's book and instance table (viekf_dispatch.hpp): included by viekf_capi.hip ONLY.
#pragma once
#include "../../include/viekf_node.h"
#include "viekf_dispatch.hpp"
#include "viekf_kernels_node.hpp"
#include "viekf_staging.hpp"

struct viekf_node {
  viekf_batch* b = nullptr;
  int device = 0;
  DevOwner own;   // the tables of t
  NodeTabs t = {};
};

namespace {

int check_node(const viekf_node* nd) {
  if (!nd || !nd->b) return fail(VIEKF_ERR_INVALID, "null node graph handle");
  return VIEKF_OK;
}

// Where the 21 elements of P that viekf_node_global reads lie IN THE FORM THE LIVE P IS IN (the book's, viekf_pform.hpp):
// canonical (Full or Lower: the lower triangle is current in both) row + column * ld, or the body block of the packed image of
// the batch's instance (ResPack, viekf_instance_rows.hpp -- the rows viekf_debug_packed_layout reports).
NodeOffs node_offsets(const viekf_batch* b) {
  const int idx[6] = {dxPOS, dxPOS + 1, dxPOS + 2, dxATT, dxATT + 1, dxATT + 2};
  NodeOffs of;
  if (b->book.live_form() == PForm::Packed) {   // (only ever left by the batch's instance of the resident family)
    const ResInst& r = kResInst[b->res_inst];
    const ResPack K(b->N, r.RB, r.NW);
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++) of.o[i * (i + 1) / 2 + j] = K.body(idx[i], idx[j]);
  } else {
    for (int i = 0; i < 6; i++)
      for (int j = 0; j <= i; j++) of.o[i * (i + 1) / 2 + j] = idx[i] + idx[j] * b->ld;
  }
  return of;
}

unsigned node_grid(const viekf_batch* b) { return (unsigned)((b->B + 63) / 64); }

}  // namespace

extern "C" {

int viekf_node_destroy(viekf_node* nd) {
  if (!nd) return fail(VIEKF_ERR_INVALID, "null node graph handle");
  (void)hipSetDevice(nd->device);
  (void)hipDeviceSynchronize();   // (not the batch's stream: the tables may be freed after their batch is gone)
  nd->own.release_all();
  delete nd;
  return VIEKF_OK;
}

int viekf_node_create(viekf_batch* b, int32_t trail_capacity, viekf_node** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (int rc = check_batch(b)) return rc;
  if (trail_capacity < 0 || trail_capacity > VIEKF_NODE_MAX_TRAIL) return fail(VIEKF_ERR_INVALID, "need 0 <= trail_capacity <= 4096");
  HIP_TRY(hipSetDevice(b->device));
  viekf_node* nd = new viekf_node();
  nd->b = b; nd->device = b->device;
  NodeTabs& t = nd->t;
  t.cap = trail_capacity;
  const size_t B = (size_t)b->B;
  DevOwner& own = nd->own;
  int rc = own.alloc(&t.node, 7 * B);
  if (!rc) rc = own.alloc(&t.cov, 36 * B);
  if (!rc) rc = own.alloc(&t.tnode, 7 * B);
  if (!rc) rc = own.alloc(&t.count, B);
  if (!rc) rc = own.alloc(&t.tr_node, 7 * B * (size_t)t.cap);
  if (!rc) rc = own.alloc(&t.tr_edge, 17 * B * (size_t)t.cap);
  if (!rc) rc = viekf_node_reset(nd);
  if (rc) { viekf_node_destroy(nd); return rc; }
  *out = nd;
  return VIEKF_OK;
}

int viekf_node_reset(viekf_node* nd) {
  if (int rc = check_node(nd)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const NodeTabs& t = nd->t;
  hipLaunchKernelGGL(k_node_reset, dim3(node_grid(b)), dim3(64), 0, b->stream, b->B, t);
  HIP_TRY(hipGetLastError());
  if (t.cap > 0) {
    HIP_TRY(hipMemsetAsync(t.tr_node, 0, sizeof(double) * 7 * (size_t)b->B * t.cap, b->stream));
    HIP_TRY(hipMemsetAsync(t.tr_edge, 0, sizeof(double) * 17 * (size_t)b->B * t.cap, b->stream));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_node_update(viekf_node* nd, const uint8_t* did_reset, const double* edges, const double* x_true, int32_t ldx, viekf_mem where) {
  if (int rc = check_node(nd)) return rc;
  if (!did_reset || !edges) return fail(VIEKF_ERR_INVALID, "did_reset and edges must not be null");
  if (x_true && ldx < 10) return fail(VIEKF_ERR_INVALID, "x_true needs ldx >= 10 (position 0:3, attitude 6:10)");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const uint8_t* d_dr = nullptr;
  const double *d_e = nullptr, *d_xt = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(did_reset, B, &d_dr), in(edges, 17 * B, &d_e), in(x_true, x_true ? B * (size_t)ldx : 0, &d_xt))) return rc;
  hipLaunchKernelGGL(k_node_update, dim3(node_grid(b)), dim3(64), 0, b->stream, b->B, nd->t, d_dr, d_e, d_xt, ldx);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

// read-only, and P is read in the form it is in: no require_P here (an unpack would cross all of P to read 21 numbers)
int viekf_node_global(viekf_node* nd, double* pose, double* cov, viekf_mem where) {
  if (int rc = check_node(nd)) return rc;
  if (!pose && !cov) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  double *d_pose = nullptr, *d_cov = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(out(pose, 7 * B, &d_pose), out(cov, 36 * B, &d_cov))) return rc;
  hipLaunchKernelGGL(k_node_global, dim3(node_grid(b)), dim3(64), 0, b->stream, make_args(b), nd->t, node_offsets(b), d_pose, d_cov);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_node_relative_truth(viekf_node* nd, const double* x_true, double* x_rel, int32_t ldx, viekf_mem where) {
  if (int rc = check_node(nd)) return rc;
  if (!x_true || !x_rel) return fail(VIEKF_ERR_INVALID, "x_true and x_rel must not be null");
  if (ldx < 10) return fail(VIEKF_ERR_INVALID, "x_true needs ldx >= 10 (position 0:3, attitude 6:10)");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t cnt = (size_t)b->B * (size_t)ldx;
  const double* d_xt = nullptr;
  double* d_xr = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(x_true, cnt, &d_xt), out(x_rel, cnt, &d_xr))) return rc;
  hipLaunchKernelGGL(k_node_relative_truth, dim3(b->B), dim3(64), 0, b->stream, b->B, nd->t, d_xt, d_xr, ldx);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_node_global_error(viekf_node* nd, const double* x_true, int32_t ldx, double* err, double* nees, int32_t* info, viekf_mem where) {
  if (int rc = check_node(nd)) return rc;
  if (!x_true) return fail(VIEKF_ERR_INVALID, "x_true must not be null");
  if (!err && !nees && !info) return fail(VIEKF_ERR_INVALID, "at least one output must not be null");
  if (ldx < 10) return fail(VIEKF_ERR_INVALID, "x_true needs ldx >= 10 (position 0:3, attitude 6:10)");
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const double* d_xt = nullptr;
  double *d_err = nullptr, *d_nees = nullptr;
  int32_t* d_info = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(x_true, B * (size_t)ldx, &d_xt), out(err, 6 * B, &d_err), out(nees, B, &d_nees), out(info, B, &d_info))) return rc;
  hipLaunchKernelGGL(k_node_global_error, dim3(node_grid(b)), dim3(64), 0, b->stream, make_args(b), nd->t, node_offsets(b), d_xt, ldx,
                     d_err, d_nees, d_info);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

static int node_copy(viekf_node* nd, bool get, void* node, void* node_cov, void* true_node, void* count, viekf_mem where) {
  if (int rc = check_node(nd)) return rc;
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const NodeTabs& t = nd->t;
  struct Arr { void* user; void* dev; size_t bytes; } arrs[] = {{node, t.node, sizeof(double) * 7 * B}, {node_cov, t.cov, sizeof(double) * 36 * B},
                                                                {true_node, t.tnode, sizeof(double) * 7 * B}, {count, t.count, sizeof(int32_t) * B}};
  for (const Arr& a : arrs)
    if (int rc = copy_user(get ? a.user : a.dev, get ? a.dev : a.user, a.bytes, where, get ? Copy::ToUser : Copy::FromUser, b->stream)) return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_node_get(viekf_node* nd, double* node, double* node_cov, double* true_node, int32_t* count, viekf_mem where) {
  return node_copy(nd, true, node, node_cov, true_node, count, where);
}

int viekf_node_set(viekf_node* nd, const double* node, const double* node_cov, const double* true_node, const int32_t* count, viekf_mem where) {
  return node_copy(nd, false, const_cast<double*>(node), const_cast<double*>(node_cov), const_cast<double*>(true_node),
                   const_cast<int32_t*>(count), where);
}

int viekf_node_trail(viekf_node* nd, double* nodes, double* edges, viekf_mem where) {
  if (int rc = check_node(nd)) return rc;
  if (int rc = check_where(where)) return rc;
  viekf_batch* b = nd->b;
  HIP_TRY(hipSetDevice(b->device));
  const size_t rows = (size_t)b->B * (size_t)nd->t.cap;
  if (rows) {
    if (int rc = copy_user(nodes, nd->t.tr_node, sizeof(double) * 7 * rows, where, Copy::ToUser, b->stream)) return rc;
    if (int rc = copy_user(edges, nd->t.tr_edge, sizeof(double) * 17 * rows, where, Copy::ToUser, b->stream)) return rc;
  }
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

}  // extern "C"
