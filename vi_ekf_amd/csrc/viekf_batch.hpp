// viekf_batch.hpp -- the batch handle of the C ABI (include/viekf.h), the error plumbing and the handle's small accessors.
// Pulls in viekf_kernels_stream.hpp (StreamArgs), which defines kernels: for the one HIP translation unit, viekf_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/viekf.h"
#include "viekf_host.hpp"
#include "viekf_kernels_stream.hpp"

using namespace viekf;

struct viekf_batch {
  int B = 0, N = 0, nx = 0, nxs = 0, n = 0, ld = 0, device = 0;
  viekf_params params;
  hipStream_t stream = nullptr;
  bool own_stream = false;
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
  // P is symmetric and the hot kernels keep only its LOWER triangle current; what is above the diagonal may be stale:
  //   0  all of P valid
  //   2  stale above the diagonal (left by the fused kernels, the matrix-core propagate and the grouped update: all of them read
  //      and write the lower triangle only)
  //   3  the live P may be PACKED: not the column-major matrix but the fused kernel's own register and LDS image (ResPack,
  //      viekf_instance_rows.hpp), left by a fused launch for the next one -- whole-batch mode only, never under per-filter
  //      live slots or a participation mask (the batch would end up mixed)
  // ensure_full_P(b, tolerate) brings the live P down to a level the caller can read: 3 -> 2 by unpacking (the fused kernel's
  // own conversion launch), 2 -> 0 by mirroring the lower triangle up.  Levels are set through set_level only.
  int upper_stale = 0;
  int stale_ever = 0;         // the highest CANONICAL level (<= 2) any launch of this batch has left: a canonical ring slot is taken
                              // to be that stale when it becomes (part of) the live state again
  // Form of every buffer that can hold a whole batch's P: packed (1) or canonical (0) -- the batch's own buffers and each ring
  // slot.  Set by whoever writes the buffer (a fused launch through P_out, ring copies, snapshot / restore), consulted when it
  // becomes live.  Launches are uniform over the batch, so this is host state; the live buffer's entry is (upper_stale == 3).
  unsigned char home_packed = 0;
  std::vector<unsigned char> slot_packed;   // [hist_depth]
  int tune_packed_p = 1;      // VIEKF_TUNE_PACKED_P: 0 = fused launches store canonical
  int hist_depth = 0;
  int live_slot = -1;        // >= 0: the live (x, P) ARE this slot of the history ring (d_x / d_P point into it)
  double *home_x = nullptr, *home_P = nullptr;   // the batch's own buffers (live state while live_slot < 0)
  double *h_x = nullptr, *h_P = nullptr;
  int* h_len = nullptr;
  unsigned char* d_active = nullptr;   // [B] participation mask of the next propagate / feature-update launches (NULL: all)
  bool active_on = false;
  int* d_resmap = nullptr;             // fused-step kernel: block ownership map [RB][TW] of the chosen instance (build_resmap)
  int* d_ringslot = nullptr;           // [B] staging of per-filter ring slots (viekf_batch_snapshot_filters / _restore_filters)
  // per-filter live ring slots (viekf_batch_select_filters): every filter's live (x, P) is a slot of the ring of its own; d_x / d_P
  // then point at the ring's base and the kernels address filter b through smap[b] = slot_b * B + b (StreamArgs::si).
  bool per_filter = false;
  std::vector<int32_t> live_slots;     // [B] host mirror
  int* d_smap = nullptr;               // [B] device: smap[b] = live_slots[b] * B + b, kept current in stream order by k_set_smap and by
                                       // the fused kernel itself when it stores a filter into another slot
  int* d_zero = nullptr;               // [B] zeros (gather / scatter between the ring and the batch's own buffers)
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
  size_t diag_ws_bytes = 0;
};

namespace {

inline int fail(int code, const std::string& msg) { return viekf::set_last_error(code, msg); }

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess)                                                                              \
      return fail(VIEKF_ERR_HIP, std::string(#expr) + " failed: " + hipGetErrorString(e_));            \
  } while (0)

int check_batch(const viekf_batch* b) {
  if (!b) return fail(VIEKF_ERR_INVALID, "null batch handle");
  return VIEKF_OK;
}

StreamArgs make_args(const viekf_batch* b) {
  StreamArgs a;
  a.smap = b->per_filter ? b->d_smap : nullptr;
  a.smap_out = nullptr;
  a.kcount = nullptr;
  a.x =b->d_x; a.P = b->d_P; a.len = b->d_len; a.flags = b->d_flags;
  a.Qx = b->d_Qx; a.lambda = b->d_lambda; a.ws = b->d_ws;
  a.B = b->B; a.N = b->N; a.nx = b->nx; a.nxs = b->nxs; a.n = b->n; a.ld = b->ld;
  a.ws_stride = b->ws_stride;
  a.dp = b->d_dp;
  a.x_out = b->d_x; a.P_out = b->d_P;
  a.active = b->active_on ? b->d_active : nullptr;
  a.resmap = b->d_resmap;
  return a;
}

// bytes of one ring slot's x / P, and where slot `slot` of the history ring starts
size_t hist_nx(const viekf_batch* b) { return sizeof(double) * (size_t)b->B * b->nxs; }
size_t hist_nP(const viekf_batch* b) { return sizeof(double) * (size_t)b->B * b->n * b->ld; }
double* slot_x(const viekf_batch* b, int slot) { return reinterpret_cast<double*>(reinterpret_cast<char*>(b->h_x) + hist_nx(b) * slot); }
double* slot_P(const viekf_batch* b, int slot) { return reinterpret_cast<double*>(reinterpret_cast<char*>(b->h_P) + hist_nP(b) * slot); }

// The packed / canonical entry of the buffer that holds the live P: a ring slot's or the batch's own buffers'.  Whole-batch mode
// only: under per-filter live slots no single buffer is live, every buffer stays canonical and there is no entry (nullptr).
unsigned char* live_form(viekf_batch* b) {
  if (b->per_filter) return nullptr;
  return b->live_slot >= 0 ? &b->slot_packed[(size_t)b->live_slot] : &b->home_packed;
}
// The one place the live level changes, in every mode: keeps the live buffer's form entry (where there is one) and stale_ever
// with it.  Callers do not branch on per_filter.
void set_level(viekf_batch* b, int level) {
  b->upper_stale = level;
  if (unsigned char* f = live_form(b)) *f = level == 3;
  b->stale_ever = std::max(b->stale_ever, std::min(level, 2));
}
// A covariance is copied into and out of the ring as it stands, stale upper triangle included.  A buffer's FORM is known
// (home_packed / slot_packed); a canonical buffer carries no level of its own: what becomes (part of) the live state again is
// taken to be as stale as anything canonical this batch ever produced.
void mark_restored_stale(viekf_batch* b) { b->upper_stale = std::min(2, std::max(b->stale_ever, b->upper_stale)); }
// ... the live P now IS (a copy of) a whole-batch buffer of form `packed` (whole-batch mode: both callers refuse per-filter mode)
void mark_live_from(viekf_batch* b, bool packed) {
  if (packed) b->upper_stale = 3; else mark_restored_stale(b);
  if (unsigned char* f = live_form(b)) *f = packed;
}

// lambda = 1 on the bearing components, or no partial update at all: the fused kernel's unit-Lambda (ZU) instances apply
bool unit_lambda(const viekf_params& p) { return !p.use_partial_update || (p.lambda_feat[0] == 1.0 && p.lambda_feat[1] == 1.0); }

}  // namespace
