// viekf_dispatch.hpp -- which kernel runs a batch and how it is launched: the instance tables, the choice of an instance when a
// batch is created (setup_resident / setup_tiles), the launches of the three families.  The headers that DEFINE kernels are
// included here (and the companions' from viekf_capi.hip), nowhere else; what several of them share -- the kernel arguments,
// the measurement models, the LDS layouts -- defines none.  So a new kernel, template or not, needs no guard: the objects of
// viekf_inst.hip include viekf_instances.hpp alone, which reaches no header with a non-template __global__.
#pragma once
#include <cstdlib>
#include <initializer_list>
#include <mutex>

#include "viekf_batch.hpp"
#include "viekf_instances.hpp"
#include "viekf_kernels_body.hpp"
#include "viekf_kernels_depth.hpp"
#include "viekf_kernels_generic.hpp"
#include "viekf_kernels_grouped.hpp"
#include "viekf_kernels_hooks.hpp"
#include "viekf_kernels_lifecycle.hpp"
#include "viekf_kernels_pixvel.hpp"
#include "viekf_kernels_stream.hpp"
#include "viekf_kernels_util.hpp"
#include "viekf_kernels_wide.hpp"

// (the fused-step kernels are compiled in viekf_inst.hip, one object file per group of instances)
#define RES_EXT(...) VIEKF_RES_FLAVOURS(extern, __VA_ARGS__)
#define TILE_EXT(...) VIEKF_TILE_FLAVOURS(extern, __VA_ARGS__)
VIEKF_RES_LIST(RES_EXT)
VIEKF_TILE_LIST(TILE_EXT)
#undef RES_EXT
#undef TILE_EXT

namespace {

constexpr int kThreads = 256;

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) belongs to a device's copy of a kernel and is shared by every batch (and
// every host thread) that launches it: a high-water mark per device (`have`, a slot of the caller's static table), raised
// under this lock and never lowered -- a second batch with fewer features must not take the first one's LDS away.
std::mutex g_attr_mutex;
template <typename Kernel>
int raise_dyn_lds(std::initializer_list<Kernel*> kernels, size_t bytes, size_t& have) {
  std::lock_guard<std::mutex> lk(g_attr_mutex);
  if (bytes <= have) return VIEKF_OK;
  for (Kernel* k : kernels)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  have = bytes;
  return VIEKF_OK;
}

// elements and strides of the measurement noise R: r_mode 0 one R for all, 1 one per filter, 2 one per filter and measurement
// (rr elements each: the 2 x 2 of a pixel measurement unless the caller has another rdim)
size_t r_count(const viekf_batch* b, int M, int r_mode, size_t rr = 4) {
  return r_mode == 0 ? rr : (r_mode == 1 ? rr * (size_t)b->B : rr * (size_t)b->B * M);
}
void r_strides(int r_mode, int M, long* rsb, long* rsm, long rr = 4) {
  *rsb = r_mode == 1 ? rr : (r_mode == 2 ? rr * M : 0);
  *rsm = r_mode == 2 ? rr : 0;
}
// (nxs, n) of a batch with num_features slots, for the *_lds_bytes entry points; false outside what they answer for
bool lds_dims(int num_features, int* nxs, int* n) {
  *nxs = (17 + 5 * num_features + 1) & ~1;
  *n = 16 + 3 * num_features;
  return num_features >= 0 && num_features <= 4096;
}

// A grouped update (k_update_feat_blocked) keeps only the lower triangle of P current; the matrix-core propagate reads only
// that and rewrites all of P; a fused launch may leave P packed.  Every reader says which form it can take: require_P, below
// the kernel tables.
int require_P(viekf_batch* b, PForm at_most);

// (VIEKF_TUNE_STREAM_MFMA = 0 keeps the kernels without matrix-core passes: experiments)
bool stream_mfma_ok(const viekf_batch* b) { return b->tune_stream_mfma != 0; }

int launch_propagate(viekf_batch* b, const double* d_u, const double* d_dt, const unsigned char* call_mask = nullptr) {
  if (int rc = require_P(b, stream_mfma_ok(b) ? PForm::Lower : PForm::Full)) return rc;
  StreamArgs a = make_args(b, call_mask);
  if (stream_mfma_ok(b)) {   // feature/feature part on the fp64 matrix cores: reads and writes the lower triangle only
    const size_t wlds = WideLds(b->N, b->nxs, sizeof(BodyCtx)).bytes();
    if (b->tune_stream_mfma != 2 && 3 * b->N <= 512 && wlds <= 158 * 1024) {   // the K = 24 record form, records in LDS
      static size_t have[64] = {};
      if (int rc = raise_dyn_lds({&k_propagate_wide<512>}, wlds, have[b->device & 63])) return rc;
      hipLaunchKernelGGL((k_propagate_wide<512>), dim3(b->B), dim3(512), wlds, b->stream, a, d_u, d_dt);
    } else {                                                                    // r02's K = 38 form, operands staged in global scratch
      hipLaunchKernelGGL((k_propagate_stream<512, true>), dim3(b->B), dim3(512), PropLds(b->nxs, sizeof(BodyCtx), b->N, true).bytes(),
                         b->stream, a, d_u, d_dt);
    }
    b->book.wrote_live(PForm::Lower);
  } else
    hipLaunchKernelGGL((k_propagate_stream<kThreads, false>), dim3(b->B), dim3(kThreads),
                       PropLds(b->nxs, sizeof(BodyCtx), b->N, false).bytes(), b->stream, a, d_u, d_dt);
  HIP_TRY(hipGetLastError());
  return VIEKF_OK;
}

// The grouped update of this batch, if any (grouped_choice, viekf_stream_lds.hpp: THE rule, with the LDS budget)
GroupedChoice grouped(const viekf_batch* b) {
  return grouped_choice(b->N, b->n, b->nxs, b->tune_block_group, b->tune_panel_svc, b->tune_stream_mfma);
}
bool panel_svc(const viekf_batch* b) { return grouped(b).kernel == GroupedKernel::panelsvc; }
int blocked_group(const viekf_batch* b) { return grouped(b).BG; }   // measurements per group; 0: one pass per measurement

int launch_update(viekf_batch* b, const double* d_z, const int* d_slot, int M, const double* d_R, int r_mode,
                  int* d_res) {
  if (int rc = require_P(b, PForm::Lower)) return rc;   // (a fused launch may have left P packed)
  StreamArgs a = make_args(b);
  long rsb = 0, rsm = 0;
  r_strides(r_mode, M, &rsb, &rsm);
  // wide P: a grouped kernel (one HBM pass over P per group of BG measurements, fp64 MFMA pass)
  const GroupedChoice gc = grouped(b);
  if (M >= 1 && gc.kernel != GroupedKernel::none) {   // (a single measurement too: a group of one, no mirror pass before it)
    typedef void (*blk_kernel_t)(StreamArgs, const double*, const int*, int, const double*, long, long, int*);
    const bool sv = gc.kernel == GroupedKernel::panelsvc;
    const int bg = gc.BG;
    const size_t blds = gc.bytes;
    const blk_kernel_t kern = sv ? k_update_feat_panelsvc<kGroupedThreads, 16>
                                 : (bg == 32 ? k_update_feat_blocked<kGroupedThreads, 32>
                                             : (bg == 24 ? k_update_feat_blocked<kGroupedThreads, 24> : k_update_feat_blocked<kGroupedThreads, 16>));
    static size_t have[64][6] = {};
    if (int rc = raise_dyn_lds({kern}, blds, have[b->device & 63][(bg == 32 ? 2 : (bg == 24 ? 1 : 0)) + (sv ? 3 : 0)])) return rc;
    hipLaunchKernelGGL(kern, dim3(b->B), dim3(kGroupedThreads), blds, b->stream, a, d_z, d_slot, M, d_R, rsb, rsm, d_res);
    b->book.wrote_live(PForm::Lower);   // (reads and writes the lower triangle only)
  } else {
    if (int rc = require_P(b, PForm::Full)) return rc;   // (the one-measurement kernel reads whole columns)
    hipLaunchKernelGGL(k_update_feat_stream<kThreads>, dim3(b->B), dim3(kThreads), UpdLds(b->nxs, b->n).bytes(), b->stream, a,
                       d_z, d_slot, M, d_R, rsb, rsm, d_res);
  }
  HIP_TRY(hipGetLastError());
  return VIEKF_OK;
}

typedef void (*res_kernel_t)(StreamArgs, int, const double*, const double*, const double*, const int*, int, int,
                             const double*, long, long, int*);
// The kernels behind the rows of kResInst / kTileInst (viekf_instance_rows.hpp), expanded from the same lists.
// multi: several propagates per launch (viekf_batch_step_n); zu: the unit-Lambda instances (both flavours: step_n must stay
// bit for bit what K propagates and a step give)
struct ResKernels { res_kernel_t k[4]; };    // [multi + 2 * zu]
struct TileKernels { res_kernel_t k[2]; };   // [multi]
#define RES_KERNELS(RB, NW, NS, ...)                                                                   \
  {{k_step_resident<RB, NW, false, NS, false>, k_step_resident<RB, NW, true, NS, false>,              \
    k_step_resident<RB, NW, false, NS, true>, k_step_resident<RB, NW, true, NS, true>}},
#define TILE_KERNELS(NT, NW, ...) \
  {{k_step_tiles_pair<NT, false>, k_step_tiles_pair<NT, true>}}, {{k_step_tiles<NT, NW, false>, k_step_tiles<NT, NW, true>}},
const ResKernels kResKernels[] = {VIEKF_RES_LIST(RES_KERNELS)};
const TileKernels kTileKernels[] = {VIEKF_TILE_LIST(TILE_KERNELS)};
#undef RES_KERNELS
#undef TILE_KERNELS
static_assert(sizeof(kResKernels) / sizeof(kResKernels[0]) == kNumResInst, "one set of kernels per row of kResInst");
static_assert(sizeof(kTileKernels) / sizeof(kTileKernels[0]) == kNumTileInst, "one set of kernels per row of kTileInst");

res_kernel_t res_kernel(int inst, bool multi, bool zu) { return kResKernels[inst].k[(multi ? 1 : 0) + (zu ? 2 : 0)]; }
res_kernel_t tile_kernel(int inst, bool multi) { return kTileKernels[inst].k[multi ? 1 : 0]; }

// May a fused launch of this batch's instance keep P packed?  THE fit rule (ResPack::fits, viekf_instance_rows.hpp).
bool packed_fits(const viekf_batch* b) {
  if (b->res_inst < 0) return false;
  const ResInst& r = kResInst[b->res_inst];
  return ResPack(b->N, r.RB, r.NW).fits(b->n, b->ld);
}

// Unpack: the packed image in (x, P) -- a whole batch's buffer, live or a ring slot -- becomes the canonical lower triangle, in
// place.  A conversion-only launch of the fused kernel itself (no propagate, M = 0, packed load, canonical store,
// RES_FMT_P_ONLY): every workgroup loads its whole image before its first store, the arithmetic between load and store is
// skipped (nothing pending), x, status and result buffers are not written -- an identity on everything but P's form.
int unpack_buffer(viekf_batch* b, double* x, double* P) {
  StreamArgs a = make_args(b);
  a.x = a.x_out = x; a.P = a.P_out = P;
  a.smap = nullptr; a.smap_out = nullptr; a.active = nullptr;
  const ResInst& r = kResInst[b->res_inst];
  hipLaunchKernelGGL(res_kernel(b->res_inst, false, b->res_zu), dim3((unsigned)b->B), dim3((r.NW + r.NS) * 64), b->res_lds, b->stream, a,
                     launch_pack(false, 1, RES_FMT_LOAD_PACKED | RES_FMT_P_ONLY, 0), nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0L, 0L, nullptr);
  HIP_TRY(hipGetLastError());
  return VIEKF_OK;
}

// Brings the live P to at most the form the caller can take -- PForm::Full for whoever reads P whole, PForm::Lower for whoever
// reads or writes elements of the lower triangle in place -- by the book's plan.  Touches the device only when it launches.
int require_P(viekf_batch* b, PForm at_most) {
  const PPlan plan = b->book.plan(at_most);
  if (!plan.unpack && !plan.mirror) return VIEKF_OK;
  HIP_TRY(hipSetDevice(b->device));
  if (plan.unpack) {
    if (int rc = unpack_buffer(b, b->d_x, b->d_P)) return rc;
    b->book.wrote_live(PForm::Lower);
  }
  if (plan.mirror) {
    StreamArgs a = make_args(b);
    const int nt = (b->n + 31) / 32;
    hipLaunchKernelGGL(k_mirror_upper, dim3((unsigned)(nt * (nt + 1) / 2), b->B), dim3(256), 0, b->stream, a);
    HIP_TRY(hipGetLastError());
    b->book.wrote_live(PForm::Full);
  }
  return VIEKF_OK;
}
// Every buffer of the batch canonical: before the ownership map changes (setup_resident) and before anything that moves single
// filters between buffers (per-filter ring copies and live slots) -- a buffer must never hold filters of both forms.
int canonicalize_all(viekf_batch* b) {
  if (int rc = require_P(b, PForm::Lower)) return rc;
  for (int i = 0; i <= b->hist_depth; i++) {   // (the ring's slots, then the batch's own buffers)
    const int buf = i < b->hist_depth ? i : PBook::kHome;
    if (!b->book.packed(buf)) continue;
    if (int rc = unpack_buffer(b, buf_x(b, buf), buf_P(b, buf))) return rc;
    b->book.unpacked(buf);
  }
  return VIEKF_OK;
}

static_assert(sizeof(BodyCtx) == kBodyCtxBytes, "tests/cpp/fused_lds_model.cpp checks the fused carve-ups with this size");

int setup_tiles(viekf_batch* b) {
  b->tile_inst = -1;
  if (!b->tune_tiles || b->N + 14 > 64 || b->N < 1) return VIEKF_OK;
  const int NT = tile_nt(b->N);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess || cus <= 0) cus = 256;
  for (int i = 0; i < kNumTileInst; i++) {
    const TileInst& r = kTileInst[i];
    if (r.NT != NT || 16 * NT > 64 * r.NW) continue;   // (one worker thread per tile-space row brings the next column pair up to date)
    // tune_tiles: 0 / 1 the resident family (on the MI355X it is the faster one at every batch size measured, so "automatic"
    // never picks a tile instance), 2 the single form, 3 the paired form -- whatever the batch size
    if (b->tune_tiles == 1) continue;
    if (b->tune_tiles == 2 && r.pair) continue;
    if (b->tune_tiles == 3 && !r.pair) continue;
    const TileLds L(b->N, b->n, b->nxs, sizeof(BodyCtx));
    const size_t lds = sizeof(double) * (size_t)L.total * (r.pair ? 2 : 1);
    if (lds > (size_t)r.max_lds_kb * 1024) continue;
    static size_t have[64][kNumTileInst] = {};
    const res_kernel_t* k = kTileKernels[i].k;
    if (int rc = raise_dyn_lds({k[0], k[1]}, lds, have[b->device & 63][i])) return rc;
    b->tile_inst = i; b->tile_lds = lds;
    break;
  }
  return VIEKF_OK;
}

int setup_resident(viekf_batch* b) {
  b->res_inst = -1;
  const bool force = b->tune_res_inst >= 0;   // (VIEKF_TUNE_RES_INSTANCE: pick an instance by index)
  for (int i = 0; i < kNumResInst; i++) {
    const ResInst& r = kResInst[i];
    if (force && b->tune_res_inst != i) continue;
    if (b->N < r.nmin || b->N > r.nmax) continue;
    if (b->N * (b->N + 1) / 2 > r.RB * r.NW * 64 || b->N > r.NW * 64) continue;
    const ResLds L(b->N, b->n, b->nxs, res_batched_loads(r.RB, r.NW), sizeof(BodyCtx));
    const size_t lds = sizeof(double) * (size_t)L.total;
    if (lds > (size_t)r.max_lds_kb * 1024) continue;
    if (r.max_lds_kb <= 80 && !force) {   // two small workgroups per CU only pay when the batch fills the CUs more than once
      int cus = 0;
      if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, b->device) != hipSuccess || cus <= 0) cus = 256;
      if (b->B <= cus) continue;
      if (r.max_lds_kb <= 40 && b->B <= 2 * cus) continue;   // (four per CU: only when two per CU would leave filters waiting)
    }
    std::vector<int> map;
    if (!build_resmap(b->N, r.RB, r.NW, map)) continue;
    if (int rc = b->own.free(&b->d_resmap)) return rc;
    if (int rc = b->own.alloc(&b->d_resmap, map.size())) return rc;
    HIP_TRY(hipMemcpy(b->d_resmap, map.data(), sizeof(int) * map.size(), hipMemcpyHostToDevice));
    static size_t have[64][kNumResInst] = {};
    const res_kernel_t* k = kResKernels[i].k;
    if (int rc = raise_dyn_lds({k[0], k[1], k[2], k[3]}, lds, have[b->device & 63][i])) return rc;
    b->res_inst = i; b->res_lds = lds;
    break;
  }
  return VIEKF_OK;
}

// Timing-only ablation (results become wrong) exists in a -DVIEKF_ABLATE diagnostic build only (tools/build_variant.sh): the
// bits 1 skip sweeps, 2 skip state correction, 4 skip the column extraction come from VIEKF_DEBUG_ABLATE there.  The product
// library has no such switch.
#ifdef VIEKF_ABLATE
int dbg_bits() {
  static const int v = []() { const char* e = getenv("VIEKF_DEBUG_ABLATE"); return e ? atoi(e) : 0; }();
  return v;
}
#else
constexpr int dbg_bits() { return 0; }
#endif

bool use_tiles(const viekf_batch* b) { return b->tile_inst >= 0 && b->family != 1; }
bool use_resident(const viekf_batch* b) { return (b->res_inst >= 0 || b->tile_inst >= 0) && b->family != 1; }

// Do this batch's fused launches keep P PACKED from one launch to the next (nobody reads the canonical matrix in between)?  Not
// the tile family, not under per-filter live slots (a buffer would end up mixed), VIEKF_TUNE_PACKED_P on, the image fits.
bool keeps_packed(const viekf_batch* b) { return !use_tiles(b) && !b->book.per_filter() && b->tune_packed_p != 0 && packed_fits(b); }

// one launch handles at most res_mcap(N) measurements; longer lists are chunked (P makes one extra HBM round trip per chunk)
int launch_resident(viekf_batch* b, bool do_prop, const double* d_u, const double* d_dt, const double* d_z,
                    const int* d_slot, int M, const double* d_R, int r_mode, int* d_res, int dst_slot = -1, int KP = 1,
                    const int* smap_out = nullptr, const int* kcount = nullptr, const unsigned char* call_mask = nullptr) {
  // dst_slot >= 0: the launch stores (x, P) into that slot of the history ring instead of in place (a single-chunk launch:
  // viekf_batch_propagate_to / _propagate_n_to); the caller makes the slot live afterwards (viekf_batch_select)
  // (the fused kernel loads the lower triangle only and stores the lower triangle only: no symmetrisation before or after)
  // Form of P: packed where the batch keeps it packed and advances as a whole (a participation mask would leave the buffer
  // mixed; call_mask comes with per-filter mode only).  The load form is whatever the live P is; everything else gets
  // canonical P first.
  const bool store_packed = keeps_packed(b) && !b->active_on;
  if (use_tiles(b) || b->book.per_filter() || b->active_on)
    if (int rc = require_P(b, PForm::Lower)) return rc;
  int fmt = (b->book.live_form() == PForm::Packed ? RES_FMT_LOAD_PACKED : 0) | (store_packed ? RES_FMT_STORE_PACKED : 0);
  StreamArgs a = make_args(b, call_mask);
  if (dst_slot >= 0) { a.x_out = slot_x(b, dst_slot); a.P_out = slot_P(b, dst_slot); }
  a.smap_out = smap_out;
  a.kcount = kcount;   // (per-filter propagate counts: the resident multi-propagate instances, KP > 1, read them; KP is their maximum)
  long rsb = 0, rsm = 0;
  r_strides(r_mode, M, &rsb, &rsm);
  const bool tiles = use_tiles(b);
  const res_kernel_t kern = tiles ? tile_kernel(b->tile_inst, KP > 1) : res_kernel(b->res_inst, KP > 1, b->res_zu);
  const bool pair = tiles && kTileInst[b->tile_inst].pair;
  const int threads = tiles ? (pair ? 512 : (kTileInst[b->tile_inst].NW + 1) * 64) : (kResInst[b->res_inst].NW + kResInst[b->res_inst].NS) * 64;
  const unsigned grid = pair ? (unsigned)((b->B + 1) / 2) : (unsigned)b->B;
  const size_t lds = tiles ? b->tile_lds : b->res_lds;
  int m0 = 0;
  do {
    const int cap = res_mcap(b->N);
    const int mc = (M - m0 < cap) ? (M - m0) : cap;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), lds, b->stream, a,
                       launch_pack(do_prop && m0 == 0, KP, fmt, dbg_bits()), d_u, d_dt, d_z ? d_z + 2L * m0 : nullptr,
                       d_slot ? d_slot + m0 : nullptr, mc, M, d_R ? d_R + rsm * m0 : nullptr, rsb, rsm,
                       d_res ? d_res + m0 : nullptr);
    HIP_TRY(hipGetLastError());
    m0 += mc;
    // (a further chunk loads what this one stored -- which is NOT the form this one loaded when the live P was packed and this
    //  launch stores canonical: a restored packed slot with the switch off, say)
    fmt = (fmt & ~RES_FMT_LOAD_PACKED) | (store_packed ? RES_FMT_LOAD_PACKED : 0);
  } while (m0 < M);
  if (dst_slot >= 0) b->book.wrote_slot(dst_slot, store_packed);   // (the caller makes it live)
  else b->book.wrote_live(store_packed ? PForm::Packed : PForm::Lower);
  return VIEKF_OK;
}

// per-filter mode: (x, P) of every filter between its live ring slot and the batch's own buffers (to_home != 0: ring -> home)
int gather_scatter_home(viekf_batch* b, int to_home) {
  if (!b->d_zero)
    if (int rc = b->own.alloc_zeroed(&b->d_zero, (size_t)b->B, b->stream)) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_ring_copy, dim3(b->B), dim3(256), 0, b->stream, a, b->home_x, b->home_P, b->d_zero, to_home, 1);
  HIP_TRY(hipGetLastError());
  return VIEKF_OK;
}

}  // namespace
