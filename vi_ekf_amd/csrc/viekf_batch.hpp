// viekf_batch.hpp -- the batch handle of the C ABI (include/viekf.h) and the handle's small accessors (the error plumbing and
// the owner of its device memory are viekf_hostkit.hpp).
// Of the device side it needs the kernel arguments only (viekf_kernel_args.hpp: StreamArgs, no kernel defined there).  HIP
// host code all the same (hipStream_t, the owner's hipMalloc): part of viekf_capi.hip's translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/viekf.h"
#include "viekf_hostkit.hpp"
#include "viekf_kernel_args.hpp"
#include "viekf_pform.hpp"

using namespace viekf;

struct viekf_batch {
  int B = 0, N = 0, nx = 0, nxs = 0, n = 0, ld = 0, device = 0;
  viekf_params params;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevOwner own;   // every device buffer below (hipMalloc); the pinned ring h_pin is the handle's own
  double *d_x = nullptr, *d_P = nullptr, *d_Qx = nullptr, *d_lambda = nullptr, *d_ws = nullptr, *d_x0 = nullptr,
         *d_Pdiag = nullptr;
  int* d_len = nullptr;
  unsigned* d_flags = nullptr;
  long ws_stride = 0;
  char* d_stage = nullptr;
  size_t stage_bytes = 0, stage_used = 0;
  int family = 0;       // requested: 0 auto, 1 streaming, 2 resident
  int res_inst = -1;    // resident instance index (-1: N not covered by the resident family)
  bool res_zu = false;  // lambda = 1 on the bearing components (or no partial update): the fused kernel's ZU instances apply
  size_t res_lds = 0;
  DevParams dp;
  DevParams* d_dp = nullptr;
  // Per-filter parameter sets (viekf_batch_set_params_filters).  Allocated by the first call that asks for them; pf_on says whether
  // the launches read them (StreamArgs::pstride = 1) or the one set above.
  bool pf_on = false;
  std::vector<viekf_params> pf_params;   // [B] host copy (what viekf_batch_get_params_filter returns)
  std::vector<DevParams> pf_dp;          // [B] host mirror of pf_d_dp
  DevParams* pf_d_dp = nullptr;          // [B]
  double *pf_d_Qx = nullptr, *pf_d_lambda = nullptr, *pf_d_Pdiag = nullptr;   // [B][n]
  double* pf_d_x0 = nullptr;             // [B][nxs]
  // form of P between launches, which buffer holds the live state, per-filter mode (viekf_pform.hpp); d_x / d_P follow it
  // through point_live() below
  PBook book;
  int tune_packed_p = 1;      // VIEKF_TUNE_PACKED_P: 0 = fused launches store canonical
  int hist_depth = 0;
  double *home_x = nullptr, *home_P = nullptr;   // the batch's own buffers (allocated by viekf_batch_create)
  double *h_x = nullptr, *h_P = nullptr;
  int* h_len = nullptr;
  unsigned char* d_active = nullptr;   // [B] participation mask of the next propagate / feature-update launches (NULL: all)
  bool active_on = false;
  int* d_resmap = nullptr;             // fused-step kernel: block ownership map [RB][TW] of the chosen instance (build_resmap)
  int* d_ringslot = nullptr;           // [B] staging of per-filter ring slots (viekf_batch_snapshot_filters / _restore_filters)
  // per-filter live ring slots (viekf_batch_select_filters): every filter's live (x, P) is a slot of the ring of its own; d_x / d_P
  // then point at the ring's base and the kernels address filter b through smap[b] = slot_b * B + b (StreamArgs::si).
  std::vector<int32_t> live_slots;     // [B] host mirror
  int* d_smap = nullptr;               // [B] device: smap[b] = live_slots[b] * B + b, kept current in stream order by k_set_smap and by
                                       // the fused kernel itself when it stores a filter into another slot
  int* d_zero = nullptr;               // [B] zeros (gather / scatter between the ring and the batch's own buffers)
  double* d_body_z = nullptr;          // [VIEKF_BODY_MAX_M][B][4] viekf_batch_update_body's M-launch route: z repacked per entry (first use)
  int pixvel_route = -1;               // viekf_batch_pixel_vels_route: -1 automatic, 0 always the M launches, 1 fused where it fits
  double* d_depth_m = nullptr;         // [4 B + 8] viekf_batch_update_depths' M-launch route: one entry's z, R, slot, result and active per filter (first use)
  // async host inputs (viekf_batch_set_async): pinned staging ring the arguments are copied into at call time
  bool async_host = false;
  char* d_pin = nullptr;       // the device's address of h_pin
  char* h_pin = nullptr;
  size_t pin_bytes = 0, pin_used = 0;
  int tile_inst = -1;          // tile family (P as MFMA accumulator tiles): index into kTileInst, -1 = not used for this batch
  size_t tile_lds = 0;
  // viekf_batch_set_tuning (tests / experiments; the defaults are what a caller gets)
  int tune_tiles = 0;          // the tile family is opt-in (measured slower than the resident family): 2 single, 3 pair
  int tune_res_inst = -1;      // >= 0: only this index of kResInst is tried
  int tune_unit_lambda = 1;    // 0: never the unit-Lambda instances
  int tune_block_group = 0;    // 16 / 24 / 32: group size of the grouped update where its panel fits
  int tune_stream_mfma = 1;    // 0: the streaming kernels without matrix-core passes
  int tune_panel_svc = 1;      // 0: the grouped update without the service wave (k_update_feat_blocked)
  // viekf_diag_consistency where the packed triangle does not fit the LDS: allocated on first use, at most 256 MiB while one
  // filter's triangle fits that (the batch is processed in chunks of filters)
  double* d_diag_ws = nullptr;
  size_t diag_ws_cap = 0;      // doubles
};

namespace {

int check_batch(const viekf_batch* b) {
  if (!b) return fail(VIEKF_ERR_INVALID, "null batch handle");
  return VIEKF_OK;
}

// call_mask: the participation mask of this one launch, in place of the handle's (the per-filter propagates)
StreamArgs make_args(const viekf_batch* b, const unsigned char* call_mask = nullptr) {
  StreamArgs a;
  a.smap = b->book.per_filter() ? b->d_smap : nullptr;
  a.smap_out = nullptr;
  a.kcount = nullptr;
  a.x =b->d_x; a.P = b->d_P; a.len = b->d_len; a.flags = b->d_flags;
  a.Qx = b->pf_on ? b->pf_d_Qx : b->d_Qx; a.lambda = b->pf_on ? b->pf_d_lambda : b->d_lambda; a.ws = b->d_ws;
  a.B = b->B; a.N = b->N; a.nx = b->nx; a.nxs = b->nxs; a.n = b->n; a.ld = b->ld;
  a.ws_stride = b->ws_stride;
  a.dp = b->pf_on ? b->pf_d_dp : b->d_dp;
  a.pstride = b->pf_on ? 1 : 0;
  a.x_out = b->d_x; a.P_out = b->d_P;
  a.active = call_mask ? call_mask : (b->active_on ? b->d_active : nullptr);
  a.resmap = b->d_resmap;
  return a;
}

// bytes of one ring slot's x / P, and where slot `slot` of the history ring starts
size_t hist_nx(const viekf_batch* b) { return sizeof(double) * (size_t)b->B * b->nxs; }
size_t hist_nP(const viekf_batch* b) { return sizeof(double) * (size_t)b->B * b->n * b->ld; }
double* slot_x(const viekf_batch* b, int slot) { return reinterpret_cast<double*>(reinterpret_cast<char*>(b->h_x) + hist_nx(b) * slot); }
double* slot_P(const viekf_batch* b, int slot) { return reinterpret_cast<double*>(reinterpret_cast<char*>(b->h_P) + hist_nP(b) * slot); }

// (x, P) of a buffer that holds a whole batch: the batch's own (PBook::kHome) or a ring slot
double* buf_x(const viekf_batch* b, int buf) { return buf < 0 ? b->home_x : slot_x(b, buf); }
double* buf_P(const viekf_batch* b, int buf) { return buf < 0 ? b->home_P : slot_P(b, buf); }
// d_x / d_P follow the book: the live buffer, or the ring's base under per-filter mode.  Called after every event that moves
// the live state (select, enter_per_filter, resized).
void point_live(viekf_batch* b) {
  b->d_x = b->book.per_filter() ? b->h_x : buf_x(b, b->book.live_slot());
  b->d_P = b->book.per_filter() ? b->h_P : buf_P(b, b->book.live_slot());
}

// lambda = 1 on the bearing components, or no partial update at all: the fused kernel's unit-Lambda (ZU) instances apply
bool unit_lambda(const viekf_params& p) { return !p.use_partial_update || (p.lambda_feat[0] == 1.0 && p.lambda_feat[1] == 1.0); }
// ... for every set a launch of this batch may read
bool unit_lambda(const viekf_batch* b) {
  if (!b->pf_on) return unit_lambda(b->params);
  return std::all_of(b->pf_params.begin(), b->pf_params.end(), [](const viekf_params& p) { return unit_lambda(p); });
}

}  // namespace
