// viekf_capi.hip -- the entry points of the C ABI declared in include/viekf.h (libviekf_hip.so), and nothing else: the batch
// handle is viekf_batch.hpp, kernel choice and launches viekf_dispatch.hpp, argument staging viekf_staging.hpp, the ownership
// map viekf_resmap.cpp; the batch's companions (diagnostics, frame intake, node graph, landmark map, flight recorder) are viekf_capi_*.hpp,
// included at the end.  The one HIP translation unit of the host side.  No CPU fallback exists on purpose.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../include/viekf_diag.h"
#include "../../include/viekf_frame.h"
#include "../../include/viekf_map.h"
#include "../../include/viekf_node.h"
#include "viekf_dispatch.hpp"
#include "viekf_kernels_diag.hpp"
#include "viekf_kernels_frame.hpp"
#include "viekf_kernels_map.hpp"
#include "viekf_kernels_node.hpp"
#include "viekf_staging.hpp"

namespace {
thread_local std::string g_last_error;
}  // namespace

int viekf::set_last_error(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

namespace {

// the device-side form of a parameter set
void fill_dev_params(DevParams& d, const viekf_params& p) {
  std::memcpy(d.Qu, p.Qu, sizeof d.Qu);
  std::memcpy(d.P0_feat, p.P0_feat, sizeof d.P0_feat);
  std::memcpy(d.cam_center, p.cam_center, sizeof d.cam_center);
  std::memcpy(d.focal, p.focal_len, sizeof d.focal);
  std::memcpy(d.q_b_c, p.q_b_c, sizeof d.q_b_c);
  std::memcpy(d.p_b_c, p.p_b_c, sizeof d.p_b_c);
  std::memcpy(d.q_b_u, p.q_b_u, sizeof d.q_b_u);
  d.min_depth = p.min_depth;
  d.use_drag_term = p.use_drag_term;
  d.use_partial_update = p.use_partial_update;
  for (int i = 0; i < 6; i++) d.sqrtQu[i] = std::sqrt(p.Qu[i] > 0.0 ? p.Qu[i] : 0.0);
}

// a set's vectors over the n error-state rows: Qx diag, lambda, initial P diagonal (vi_ekf.cpp:134-146)
void fill_row_vectors(const viekf_params& p, int N, double* Qx, double* lam, double* Pd) {
  for (int i = 0; i < 16; i++) { Qx[i] = p.Qx[i]; lam[i] = p.lambda[i]; Pd[i] = p.P0[i]; }
  for (int i = 0; i < N; i++)
    for (int k = 0; k < 3; k++) {
      Qx[16 + 3 * i + k] = p.Qx_feat[k];
      lam[16 + 3 * i + k] = p.lambda_feat[k];
      Pd[16 + 3 * i + k] = p.P0_feat[k];
    }
}

}  // namespace

extern "C" {

int viekf_abi_version(void) { return VIEKF_ABI_VERSION; }

const char* viekf_last_error(void) { return g_last_error.c_str(); }

int viekf_device_count(int32_t* count) {
  if (!count) return fail(VIEKF_ERR_INVALID, "count is null");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) { (void)hipGetLastError(); c = 0; }
  *count = c;
  return VIEKF_OK;
}

int viekf_params_default(viekf_params* p) {
  if (!p) return fail(VIEKF_ERR_INVALID, "params is null");
  std::memset(p, 0, sizeof(*p));
  p->x0[6] = 1.0;
  p->q_b_c[0] = 1.0;
  p->q_b_u[0] = 1.0;
  p->focal_len[0] = p->focal_len[1] = 1.0;
  for (int i = 0; i < 16; i++) p->lambda[i] = 1.0;
  for (int i = 0; i < 3; i++) p->lambda_feat[i] = 1.0;
  p->min_depth = 1.5;
  p->keyframe_overlap_threshold = 0.8;
  p->use_drag_term = 1;
  p->use_partial_update = 1;
  p->use_keyframe_reset = 1;
  std::snprintf(p->name, sizeof p->name, "ekf");
  return VIEKF_OK;
}

// VIEKF::load, reference src/vi_ekf/vi_ekf.cpp:101-131 (same keys, same required lengths)
int viekf_params_load_yaml(const char* path, viekf_params* p) {
  if (!path || !p) return fail(VIEKF_ERR_INVALID, "null argument");
  viekf_params_default(p);
  YamlMap m;
  std::string err, name;
  if (!yaml_parse_file(path, m, err)) return fail(VIEKF_ERR_YAML, err);
  double v = 0.0;
#define GET(key, dst, cnt) \
  if (!yaml_get_doubles(m, key, dst, cnt, err)) return fail(VIEKF_ERR_YAML, std::string(path) + ": " + err)
  if (!yaml_get_string(m, "name", name, err)) return fail(VIEKF_ERR_YAML, std::string(path) + ": " + err);
  std::snprintf(p->name, sizeof p->name, "%s", name.c_str());
  GET("min_depth", &p->min_depth, 1);
  GET("keyframe_overlap_threshold", &p->keyframe_overlap_threshold, 1);
  GET("use_drag_term", &v, 1); p->use_drag_term = v != 0.0;
  GET("use_partial_update", &v, 1); p->use_partial_update = v != 0.0;
  GET("use_keyframe_reset", &v, 1); p->use_keyframe_reset = v != 0.0;
  GET("x0", p->x0, 17);
  GET("P0", p->P0, 16);
  GET("Qx", p->Qx, 16);
  GET("Qu", p->Qu, 6);
  GET("lambda", p->lambda, 16);
  GET("P0_feat", p->P0_feat, 3);
  GET("Qx_feat", p->Qx_feat, 3);
  GET("lambda_feat", p->lambda_feat, 3);
  GET("cam_center", p->cam_center, 2);
  GET("focal_len", p->focal_len, 2);
  GET("q_b_c", p->q_b_c, 4);
  GET("p_b_c", p->p_b_c, 3);
  GET("q_b_u", p->q_b_u, 4);
#undef GET
  return VIEKF_OK;
}

int viekf_batch_create(int32_t batch, int32_t num_features, const viekf_params* p, int32_t device,
                       viekf_batch** out) {
  if (!p || !out) return fail(VIEKF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (batch <= 0 || num_features < 0 || num_features > 4096)
    return fail(VIEKF_ERR_INVALID, "batch must be > 0 and 0 <= num_features <= 4096");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(VIEKF_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  }
  if (device < 0 || device >= ndev) return fail(VIEKF_ERR_NO_DEVICE, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  viekf_batch* b = new viekf_batch();
  b->B = batch; b->N = num_features; b->device = device;
  b->nx = 17 + 5 * num_features;
  b->n = 16 + 3 * num_features;
  b->nxs = (b->nx + 1) & ~1;
  // Column stride of P.  The streaming family (N > 77: P crosses HBM several times per step) gets columns that start on whole 128-B
  // lines, so that the 16 rows of a tile column are ONE line instead of parts of two: tools/micro/cu_stream_rate moves 6.4 instead
  // of 5.2 TB/s with the wide-P pass's access pattern, the N = 150 step went from 5.66 to 5.3 ms.  The on-chip family reads and
  // writes P once per launch and is 0.9 % SLOWER with padded columns at N = 50 (0.3495 against 0.3464 ms, three alternating runs
  // of each on one box: 239 instead of 226 MB of P next to the 256 MiB Infinity Cache): it keeps the dense stride.
  b->ld = cov_ld(num_features);   // (N > 77: columns on whole lines; viekf_host.hpp)
  b->params = *p;
  fill_dev_params(b->dp, *p);
  const WsLayout L(b->N, b->n);
  b->ws_stride = L.total;
  DevOwner& own = b->own;
  const size_t Bz = (size_t)batch, nz = (size_t)b->n;
  int rc = own.alloc(&b->home_x, Bz * b->nxs);
  if (!rc) rc = own.alloc(&b->home_P, Bz * nz * b->ld);
  if (!rc) rc = own.alloc(&b->d_Qx, nz);
  if (!rc) rc = own.alloc(&b->d_lambda, nz);
  if (!rc) rc = own.alloc(&b->d_Pdiag, nz);
  if (!rc) rc = own.alloc(&b->d_x0, 17);
  if (!rc) rc = own.alloc(&b->d_ws, Bz * (size_t)b->ws_stride);
  if (!rc) rc = own.alloc(&b->d_len, Bz);
  if (!rc) rc = own.alloc(&b->d_flags, Bz);
  if (!rc) rc = own.alloc(&b->d_dp, 1);
  if (rc) {
    viekf_batch_destroy(b);
    return rc;
  }
  point_live(b);
  hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    viekf_batch_destroy(b);
    return fail(VIEKF_ERR_HIP, std::string("hipStreamCreate failed: ") + hipGetErrorString(e));
  }
  b->own_stream = true;
  // shared per-batch vectors: Qx diag, lambda, initial P diagonal (vi_ekf.cpp:134-146)
  std::vector<double> Qx(b->n), lam(b->n), Pd(b->n);
  fill_row_vectors(*p, b->N, Qx.data(), lam.data(), Pd.data());
  auto up = [&](double* dptr, const double* h, size_t cnt) {
    if (hipMemcpy(dptr, h, cnt * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) rc = VIEKF_ERR_HIP;
  };
  up(b->d_Qx, Qx.data(), b->n);
  up(b->d_lambda, lam.data(), b->n);
  up(b->d_Pdiag, Pd.data(), b->n);
  up(b->d_x0, p->x0, 17);
  if (hipMemcpy(b->d_dp, &b->dp, sizeof(DevParams), hipMemcpyHostToDevice) != hipSuccess) rc = VIEKF_ERR_HIP;
  b->res_zu = unit_lambda(*p);
  if (rc == VIEKF_OK) rc = setup_resident(b);
  if (rc == VIEKF_OK) rc = setup_tiles(b);
  if (rc == VIEKF_OK) rc = viekf_batch_reset(b);
  if (rc != VIEKF_OK) {
    viekf_batch_destroy(b);
    return rc == VIEKF_ERR_HIP ? fail(rc, "parameter upload failed") : rc;
  }
  *out = b;
  return VIEKF_OK;
}

int viekf_batch_destroy(viekf_batch* b) {
  if (!b) return VIEKF_OK;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  b->own.release_all();
  if (b->h_pin) (void)hipHostFree(b->h_pin);
  if (b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return VIEKF_OK;
}

int viekf_batch_reset(viekf_batch* b) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  StreamArgs a = make_args(b);
  if (b->pf_on)
    hipLaunchKernelGGL(k_reset, dim3(b->B), dim3(256), 0, b->stream, a, b->pf_d_x0, b->pf_d_Pdiag, (long)b->nxs, (long)b->n);
  else
    hipLaunchKernelGGL(k_reset, dim3(b->B), dim3(256), 0, b->stream, a, b->d_x0, b->d_Pdiag, 0L, 0L);
  HIP_TRY(hipGetLastError());
  b->book.wrote_live(PForm::Full);   // (k_reset writes all of P)
  HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_batch_dims(const viekf_batch* b, int32_t* batch, int32_t* num_features, int32_t* nx, int32_t* n) {
  if (int rc = check_batch(b)) return rc;
  if (batch) *batch = b->B;
  if (num_features) *num_features = b->N;
  if (nx) *nx = b->nx;
  if (n) *n = b->n;
  return VIEKF_OK;
}

int viekf_batch_describe(const viekf_batch* b, char* out, int32_t cap) {
  if (int rc = check_batch(b)) return rc;
  if (!out || cap < 1) return fail(VIEKF_ERR_INVALID, "describe: no buffer");
  char buf[256];
  if (use_tiles(b)) {
    const TileInst& r = kTileInst[b->tile_inst];
    snprintf(buf, sizeof buf, "%s<%d>: P as %d 16x16 fp64-MFMA accumulator tiles on %d worker waves + 1 service wave per filter, %s (LDS %zu KB)",
             r.pair ? "k_step_tiles_pair" : "k_step_tiles", r.NT, r.NT * (r.NT + 1) / 2, r.NW,
             r.pair ? "two filters per 512-thread workgroup half a phase out of step, one workgroup per CU" : "one filter per 256-thread workgroup, 2 workgroups per CU",
             b->tile_lds / 1024);
  } else if (use_resident(b)) {
    const ResInst& r = kResInst[b->res_inst];
    snprintf(buf, sizeof buf, "k_step_resident<%d,%d>%s: %d worker waves x %d blocks + %d service wave%s, %s per CU (LDS %zu KB)",
             r.RB, r.NW, b->res_zu ? " ZU" : "", r.NW, r.RB, r.NS, r.NS > 1 ? "s" : "",
             r.max_lds_kb <= 40 ? "4 workgroups" : (r.max_lds_kb <= 80 ? "2 workgroups" : "1 workgroup"), b->res_lds / 1024);
    const size_t len = strlen(buf);
    snprintf(buf + len, sizeof buf - len, "; P %s between launches",
             keeps_packed(b) ? "packed" : "canonical");
  } else {
    const int bg = blocked_group(b);
    if (bg > 0)
      snprintf(buf, sizeof buf, "%s + %s<512,%d> (P in HBM/L2, one pass per group of %d measurements, fp64 MFMA "
               "passes, lower triangle only)", (b->tune_stream_mfma != 2 && 3 * b->N <= 512) ? "k_propagate_wide (K = 24 records in LDS)" : "k_propagate_stream",
               panel_svc(b) ? "k_update_feat_panelsvc" : "k_update_feat_blocked", bg, bg);
    else
      snprintf(buf, sizeof buf, "k_propagate_stream + k_update_feat_stream (P in HBM/L2, one pass per measurement)");
  }
  snprintf(out, (size_t)cap, "%s", buf);
  return VIEKF_OK;
}

int viekf_batch_get_params(const viekf_batch* b, viekf_params* out) {
  if (!b || !out) return fail(VIEKF_ERR_INVALID, "null argument");
  *out = b->params;
  return VIEKF_OK;
}

int viekf_batch_get_params_filter(const viekf_batch* b, int32_t filter, viekf_params* out) {
  if (!b || !out) return fail(VIEKF_ERR_INVALID, "null argument");
  if (filter < 0 || filter >= b->B) return fail(VIEKF_ERR_INVALID, "get_params_filter: filter index out of range");
  *out = b->pf_on ? b->pf_params[(size_t)filter] : b->params;
  return VIEKF_OK;
}

int viekf_batch_set_params_filters(viekf_batch* b, const viekf_params* p) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if (!p) {   // back to the creation set: launches from here on read the batch's one set again (the arguments say which)
    b->pf_on = false;
    b->res_zu = b->tune_unit_lambda && unit_lambda(b);
    return VIEKF_OK;
  }
  const size_t Bz = (size_t)b->B, nz = (size_t)b->n, xz = (size_t)b->nxs;
  for (size_t f = 0; f < Bz; f++) {   // every entry is checked before anything changes
    const char* field = nullptr;
    if ((p[f].use_drag_term != 0) != (b->params.use_drag_term != 0)) field = "use_drag_term";
    else if ((p[f].use_partial_update != 0) != (b->params.use_partial_update != 0)) field = "use_partial_update";
    else if ((p[f].use_keyframe_reset != 0) != (b->params.use_keyframe_reset != 0)) field = "use_keyframe_reset";
    else if (!(p[f].keyframe_overlap_threshold == b->params.keyframe_overlap_threshold)) field = "keyframe_overlap_threshold";
    if (field)
      return fail(VIEKF_ERR_INVALID, "set_params_filters: filter " + std::to_string(f) + ": " + field +
                                         " differs from the batch's (structural fields are one value per batch)");
  }
  if (!b->pf_d_dp) {   // first use: a batch that never asks for per-filter sets pays nothing
    DevParams* d_dp = nullptr;
    double *d_Qx = nullptr, *d_lam = nullptr, *d_Pd = nullptr, *d_x0 = nullptr;
    int rc = b->own.alloc(&d_dp, Bz);
    if (!rc) rc = b->own.alloc(&d_Qx, Bz * nz);
    if (!rc) rc = b->own.alloc(&d_lam, Bz * nz);
    if (!rc) rc = b->own.alloc(&d_Pd, Bz * nz);
    if (!rc) rc = b->own.alloc(&d_x0, Bz * xz);
    if (rc) return rc;   // (what was allocated stays the owner's until destroy; the batch is unchanged)
    b->pf_d_dp = d_dp; b->pf_d_Qx = d_Qx; b->pf_d_lambda = d_lam; b->pf_d_Pdiag = d_Pd; b->pf_d_x0 = d_x0;
  }
  std::vector<DevParams> dps(Bz);
  std::vector<double> Qx(Bz * nz), lam(Bz * nz), Pd(Bz * nz), x0(Bz * xz, 0.0);
  for (size_t f = 0; f < Bz; f++) {
    fill_dev_params(dps[f], p[f]);
    fill_row_vectors(p[f], b->N, &Qx[f * nz], &lam[f * nz], &Pd[f * nz]);
    std::memcpy(&x0[f * xz], p[f].x0, sizeof p[f].x0);
  }
  // in stream order behind the launches already queued (they may be reading the previous sets from these buffers)
  HIP_TRY(hipMemcpyAsync(b->pf_d_dp, dps.data(), Bz * sizeof(DevParams), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(b->pf_d_Qx, Qx.data(), Bz * nz * sizeof(double), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(b->pf_d_lambda, lam.data(), Bz * nz * sizeof(double), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(b->pf_d_Pdiag, Pd.data(), Bz * nz * sizeof(double), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipMemcpyAsync(b->pf_d_x0, x0.data(), Bz * xz * sizeof(double), hipMemcpyHostToDevice, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));   // (pageable host memory: the copies have read it when this returns)
  b->pf_params.assign(p, p + Bz);
  b->pf_dp.swap(dps);
  b->pf_on = true;
  b->res_zu = b->tune_unit_lambda && unit_lambda(b);
  return VIEKF_OK;
}

int viekf_batch_set_stream(viekf_batch* b, void* hip_stream) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (b->own_stream && b->stream) { HIP_TRY(hipStreamDestroy(b->stream)); b->stream = nullptr; b->own_stream = false; }
  // NULL is HIP's default (null) stream, exactly as a hipStream_t of 0 means everywhere else
  b->stream = static_cast<hipStream_t>(hip_stream);
  b->own_stream = false;
  return VIEKF_OK;
}

int viekf_batch_sync(viekf_batch* b) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_batch_set_async(viekf_batch* b, int32_t async_host) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  b->async_host = async_host != 0;
  return VIEKF_OK;
}

int viekf_batch_set_kernel(viekf_batch* b, int32_t family) {
  if (int rc = check_batch(b)) return rc;
  if (family < 0 || family > 2) return fail(VIEKF_ERR_INVALID, "kernel family must be 0, 1 or 2");
  if (family == 2 && b->res_inst < 0 && b->tile_inst < 0)
    return fail(VIEKF_ERR_UNSUPPORTED, "resident kernel family does not cover this num_features (1..77)");
  b->family = family;
  return VIEKF_OK;
}

int viekf_batch_set_tuning(viekf_batch* b, int32_t key, int32_t value) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  switch (key) {
    case VIEKF_TUNE_RES_INSTANCE:
      if (value < -1 || value >= kNumResInst) return fail(VIEKF_ERR_INVALID, "no such resident instance");
      if (int rc = canonicalize_all(b)) return rc;   // (a packed image is defined by the instance's ownership map: gone below)
      b->tune_res_inst = value;
      break;
    case VIEKF_TUNE_PACKED_P:
      if (int rc = require_P(b, PForm::Lower)) return rc;   // (ring slots keep their form: it is recorded per slot)
      b->tune_packed_p = value != 0;
      return VIEKF_OK;
    case VIEKF_TUNE_UNIT_LAMBDA:
      b->tune_unit_lambda = value != 0;
      b->res_zu = b->tune_unit_lambda && unit_lambda(b);
      return VIEKF_OK;
    case VIEKF_TUNE_BLOCK_GROUP:
      if (value != 0 && value != 16 && value != 24 && value != 32) return fail(VIEKF_ERR_INVALID, "group size must be 0 (auto), 16, 24 or 32");
      b->tune_block_group = value;
      return VIEKF_OK;
    case VIEKF_TUNE_PANEL_SERVICE:
      b->tune_panel_svc = value != 0;
      return VIEKF_OK;
    case VIEKF_TUNE_TILES:
      if (value < 0 || value > 3) return fail(VIEKF_ERR_INVALID, "tile family: 0 off, 1 automatic, 2 single form, 3 paired form");
      b->tune_tiles = value;
      HIP_TRY(hipStreamSynchronize(b->stream));
      return setup_tiles(b);
    case VIEKF_TUNE_STREAM_MFMA:
      if (value < 0 || value > 2) return fail(VIEKF_ERR_INVALID, "stream MFMA: 0 off, 1 on, 2 on with r02's scratch-staged propagate");
      b->tune_stream_mfma = value;
      if (!b->tune_stream_mfma) { if (int rc = require_P(b, PForm::Full)) return rc; }   // (the plain kernels read all of P)
      return VIEKF_OK;
    default:
      return fail(VIEKF_ERR_INVALID, "unknown tuning key");
  }
  HIP_TRY(hipStreamSynchronize(b->stream));   // (the ownership map of the old instance may still be in use)
  if (int rc = setup_resident(b)) return rc;
  if (b->tune_res_inst >= 0 && b->res_inst < 0) {
    b->tune_res_inst = -1;
    if (int rc = setup_resident(b)) return rc;
    return fail(VIEKF_ERR_UNSUPPORTED, "this resident instance does not hold the batch's num_features");
  }
  return VIEKF_OK;
}

int viekf_batch_get_state(viekf_batch* b, double* x, double* P, int32_t* len_features, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const hipMemcpyKind kind = where == VIEKF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const double *sx = b->d_x, *sP = b->d_P;
  if (P) if (int rc = require_P(b, PForm::Full)) return rc;
  if (b->book.per_filter() && (x || P)) {   // every filter's live slot -> the batch's own buffers, then out as usual
    if (int rc = gather_scatter_home(b, 1)) return rc;
    sx = b->home_x; sP = b->home_P;
  }
  if (x)
    HIP_TRY(hipMemcpy2DAsync(x, sizeof(double) * b->nx, sx, sizeof(double) * b->nxs, sizeof(double) * b->nx, b->B,
                             kind, b->stream));
  if (P)
    HIP_TRY(hipMemcpy2DAsync(P, sizeof(double) * b->n, sP, sizeof(double) * b->ld, sizeof(double) * b->n,
                             (size_t)b->B * b->n, kind, b->stream));
  if (len_features) HIP_TRY(hipMemcpyAsync(len_features, b->d_len, sizeof(int32_t) * b->B, kind, b->stream));
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_batch_set_state(viekf_batch* b, const double* x, const double* P, const int32_t* len_features,
                          viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const hipMemcpyKind kind = where == VIEKF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  if (len_features && where == VIEKF_HOST)
    for (int i = 0; i < b->B; i++)
      if (len_features[i] < 0 || len_features[i] > b->N)
        return fail(VIEKF_ERR_INVALID, "len_features out of range");
  double *tx = b->d_x, *tP = b->d_P;
  if (b->book.per_filter() && (x || P)) {   // through the batch's own buffers: what is not given keeps its value
    if (int rc = require_P(b, PForm::Full)) return rc;
    if (int rc = gather_scatter_home(b, 1)) return rc;
    tx = b->home_x; tP = b->home_P;
  }
  if (x)
    HIP_TRY(hipMemcpy2DAsync(tx, sizeof(double) * b->nxs, x, sizeof(double) * b->nx, sizeof(double) * b->nx, b->B,
                             kind, b->stream));
  if (P)
    HIP_TRY(hipMemcpy2DAsync(tP, sizeof(double) * b->ld, P, sizeof(double) * b->n, sizeof(double) * b->n,
                             (size_t)b->B * b->n, kind, b->stream));
  if (b->book.per_filter() && (x || P))
    if (int rc = gather_scatter_home(b, 0)) return rc;
  if (len_features) HIP_TRY(hipMemcpyAsync(b->d_len, len_features, sizeof(int32_t) * b->B, kind, b->stream));
  if (P) {
    // the kernels keep P exactly symmetric and rely on it (their rank-2 update equals the reference's Joseph form only then);
    // a NaN in the active block (the new feature counts) raises VIEKF_FLAG_NAN
    StreamArgs a = make_args(b);
    const long tot = (long)b->n * b->n;
    hipLaunchKernelGGL(k_symmetrize, dim3((unsigned)((tot + 255) / 256), b->B), dim3(256), 0, b->stream, a);
    HIP_TRY(hipGetLastError());
    b->book.wrote_live(PForm::Full);   // (all of P was given)
  }
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_batch_get_status(viekf_batch* b, uint32_t* flags, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!flags) return fail(VIEKF_ERR_INVALID, "flags is null");
  HIP_TRY(hipSetDevice(b->device));
  const hipMemcpyKind kind = where == VIEKF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(hipMemcpyAsync(flags, b->d_flags, sizeof(uint32_t) * b->B, kind, b->stream));
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(b->stream));
  return VIEKF_OK;
}

int viekf_batch_propagate(viekf_batch* b, const double* u, const double* dt, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || !dt) return fail(VIEKF_ERR_INVALID, "u and dt must not be null");
  HIP_TRY(hipSetDevice(b->device));
  const double *d_u = nullptr, *d_dt = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(u, (size_t)6 * b->B, &d_u), in(dt, (size_t)b->B, &d_dt))) return rc;
  if (use_resident(b)) {
    if (int rc = launch_resident(b, true, d_u, d_dt, nullptr, nullptr, 0, nullptr, 0, nullptr)) return rc;
  } else {
    if (int rc = launch_propagate(b, d_u, d_dt)) return rc;
  }
  return st.finish(true);
}

int viekf_batch_init_feature(viekf_batch* b, const double* pix, const double* depth, const uint8_t* mask, int32_t* ok,
                             viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!pix) return fail(VIEKF_ERR_INVALID, "pix must not be null");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;   // (writes the new feature's rows and columns in place)
  const double *d_pix = nullptr, *d_depth = nullptr;
  const uint8_t* d_mask = nullptr;
  int* d_ok = nullptr;
  const size_t B = (size_t)b->B;
  Staged st(b, where);
  if (int rc = st.begin(in(pix, 2 * B, &d_pix), in(depth, B, &d_depth), in(mask, B, &d_mask), out(ok, B, &d_ok))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_init_feature<kThreads>, dim3(b->B), dim3(kThreads), 0, b->stream, a, d_pix, d_depth, d_mask,
                     d_ok);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

static int update_or_step(viekf_batch* b, const double* u, const double* dt, bool with_propagate, const double* z,
                          const int32_t* slot, int32_t M, const double* R, int32_t r_mode, int32_t* result,
                          viekf_mem where, int K = 1) {
  if (int rc = check_batch(b)) return rc;
  if (K < 1 || K > 64) return fail(VIEKF_ERR_INVALID, "1 <= K <= 64 propagates per call");
  if (M < 0) return fail(VIEKF_ERR_INVALID, "M must be >= 0");
  if (r_mode < 0 || r_mode > 2) return fail(VIEKF_ERR_INVALID, "r_mode must be 0, 1 or 2");
  if (M > 0 && (!z || !slot || !R)) return fail(VIEKF_ERR_INVALID, "z, slot and R must not be null when M > 0");
  if (with_propagate && (!u || !dt)) return fail(VIEKF_ERR_INVALID, "u and dt must not be null");
  HIP_TRY(hipSetDevice(b->device));
  const size_t BM = (size_t)b->B * (size_t)M;
  const double *d_u = nullptr, *d_dt = nullptr, *d_z = nullptr, *d_R = nullptr;
  const int32_t* d_slot = nullptr;
  int32_t* d_res = nullptr;
  if (!with_propagate) u = dt = nullptr;
  if (M == 0) { z = R = nullptr; slot = nullptr; result = nullptr; }   // (nothing to stage, nothing to hand back)
  Staged st(b, where);
  if (int rc = st.begin(in(u, (size_t)6 * b->B * K, &d_u), in(dt, (size_t)b->B * K, &d_dt), in(z, 2 * BM, &d_z), in(slot, BM, &d_slot),
                        in(R, r_count(b, M, r_mode), &d_R), out(result, BM, &d_res)))
    return rc;
  if (use_resident(b)) {
    if (with_propagate || M > 0)
      if (int rc = launch_resident(b, with_propagate, d_u, d_dt, d_z, d_slot, M, d_R, r_mode, d_res, -1, K)) return rc;
  } else {
    if (with_propagate)
      for (int k = 0; k < K; k++)
        if (int rc = launch_propagate(b, d_u + (size_t)6 * b->B * k, d_dt + (size_t)b->B * k)) return rc;
    if (M > 0)
      if (int rc = launch_update(b, d_z, d_slot, M, d_R, r_mode, d_res)) return rc;
  }
  return st.finish(true);   // (with a result to hand back there is no skipping the synchronise)
}

// diagnostic hook (not part of include/viekf.h): first `count` 8-byte words of the device workspace
int viekf_debug_read_ws(viekf_batch* b, void* out, int count) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  HIP_TRY(hipMemcpy(out, b->d_ws, (size_t)count * 8, hipMemcpyDeviceToHost));
  return VIEKF_OK;
}

int viekf_batch_keep_features(viekf_batch* b, const uint8_t* keep, int32_t* new_len, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (int rc = require_P(b, PForm::Full)) return rc;
  if (!keep) return fail(VIEKF_ERR_INVALID, "keep must not be null");
  HIP_TRY(hipSetDevice(b->device));
  const size_t BN = (size_t)b->B * b->N;
  const uint8_t* d_keep = nullptr;
  int32_t* d_nl = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(keep, BN, &d_keep), out(new_len, (size_t)b->B, &d_nl))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_keep_features<kThreads>, dim3(b->B), dim3(kThreads), KeepLds(b->n).bytes(), b->stream, a, d_keep, d_nl);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_keyframe_reset(viekf_batch* b, const uint8_t* mask, double* edge, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (int rc = require_P(b, PForm::Full)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const uint8_t* d_mask = nullptr;
  double* d_edge = nullptr;
  Staged st(b, where);   // (a host caller's edge is zero-filled first: filters outside the mask report zeros)
  if (int rc = st.begin(in(mask, (size_t)b->B, &d_mask), out_zeroed(edge, 17 * (size_t)b->B, &d_edge))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_keyframe_reset<kThreads>, dim3(b->B), dim3(kThreads), 0, b->stream, a, d_mask, d_edge);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

// ---- read-only evaluations for the log writer (see the kernels) ----
int viekf_batch_eval_xdot(viekf_batch* b, const double* u, double* xdot, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || !xdot) return fail(VIEKF_ERR_INVALID, "u / xdot is null");
  HIP_TRY(hipSetDevice(b->device));
  const double* d_u = nullptr;
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(u, 6 * (size_t)b->B, &d_u), out(xdot, (size_t)b->B * b->n, &d_o))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_eval_xdot<kThreads>, dim3(b->B), dim3(kThreads), XdotLds(b->nxs, sizeof(BodyCtx)).bytes(), b->stream, a, d_u, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_eval_h(viekf_batch* b, int32_t type, const int32_t* slot, double* zhat, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!zhat) return fail(VIEKF_ERR_INVALID, "zhat is null");
  if (type < 0 || type > 9 || type == 7) return fail(VIEKF_ERR_INVALID, "no measurement model for this type");
  const bool needs_slot = type == 5 || type == 6 || type == 8 || type == 9;
  if (needs_slot && !slot) return fail(VIEKF_ERR_INVALID, "this measurement model needs a feature slot");
  HIP_TRY(hipSetDevice(b->device));
  const int32_t* d_slot = nullptr;
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(needs_slot ? slot : nullptr, (size_t)b->B, &d_slot), out(zhat, 4 * (size_t)b->B, &d_o))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_eval_h, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, a, type, d_slot, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

// ---- run-time drag switch (VIEKF::set_drag_term / get_drag_term, include/vi_ekf.h:290-291) ----
int viekf_batch_set_drag_term(viekf_batch* b, int32_t use_drag_term) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  b->params.use_drag_term = use_drag_term != 0;
  b->dp.use_drag_term = use_drag_term != 0;
  // (every kernel reads the flag from the device-resident parameter block at launch: ordered on the batch's stream)
  HIP_TRY(hipMemcpyAsync(b->d_dp, &b->dp, sizeof(DevParams), hipMemcpyHostToDevice, b->stream));
  if (!b->pf_dp.empty()) {   // every filter's set (in force or not: viekf_batch_set_params_filters(NULL) keeps the buffers)
    for (auto& d : b->pf_dp) d.use_drag_term = use_drag_term != 0;
    for (auto& q : b->pf_params) q.use_drag_term = use_drag_term != 0;
    HIP_TRY(hipMemcpyAsync(b->pf_d_dp, b->pf_dp.data(), b->pf_dp.size() * sizeof(DevParams), hipMemcpyHostToDevice, b->stream));
  }
  HIP_TRY(hipStreamSynchronize(b->stream));   // (b->dp is pageable host memory: the copy has read it when this returns)
  return VIEKF_OK;
}
int viekf_batch_get_drag_term(const viekf_batch* b, int32_t* use_drag_term) {
  if (!b || !use_drag_term) return fail(VIEKF_ERR_INVALID, "null argument");
  *use_drag_term = b->params.use_drag_term;
  return VIEKF_OK;
}

// ---- the reference's public test hooks, evaluated on the device (viekf_kernels_hooks.hpp) ----
int viekf_batch_eval_jacobians(viekf_batch* b, const double* x, const double* u, double* xdot, double* A, double* G, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || (!xdot && !A && !G)) return fail(VIEKF_ERR_INVALID, "u and at least one output must not be null");
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B, n = (size_t)b->n;
  const double *d_x = nullptr, *d_u = nullptr;
  double *d_xd = nullptr, *d_A = nullptr, *d_G = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(x, B * b->nx, &d_x), in(u, 6 * B, &d_u), out(xdot, B * n, &d_xd), out(A, B * n * n, &d_A), out(G, B * n * 6, &d_G)))
    return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_eval_jacobians, dim3(b->B), dim3(256), 0, b->stream, a, d_x, d_u, d_xd, d_A, d_G);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_eval_h_jacobian(viekf_batch* b, const double* x, int32_t type, const int32_t* slot, double* zhat, double* H, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!zhat || !H) return fail(VIEKF_ERR_INVALID, "zhat / H is null");
  if (type < 0 || type > 9 || type == 7) return fail(VIEKF_ERR_INVALID, "no measurement model for this type");
  const bool needs_slot = type == 5 || type == 6 || type == 8 || type == 9;
  if (needs_slot && !slot) return fail(VIEKF_ERR_INVALID, "this measurement model needs a feature slot");
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const double* d_x = nullptr;
  const int32_t* d_slot = nullptr;
  double *d_z = nullptr, *d_H = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(x, B * b->nx, &d_x), in(needs_slot ? slot : nullptr, B, &d_slot), out(zhat, 4 * B, &d_z), out(H, 3 * B * b->n, &d_H)))
    return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_eval_H, dim3((b->B + 63) / 64), dim3(64), 0, b->stream, a, d_x, type, d_slot, d_z, d_H);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

static int boxop(viekf_batch* b, int minus, const double* x1, const double* v, double* res, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!x1 || !v || !res) return fail(VIEKF_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(b->device));
  const size_t nstate = (size_t)b->B * b->nx, ntangent = (size_t)b->B * b->n;   // boxminus: state, state -> tangent
  const double *d_x1 = nullptr, *d_v = nullptr;
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(x1, nstate, &d_x1), in(v, minus ? nstate : ntangent, &d_v), out(res, minus ? ntangent : nstate, &d_o))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_boxops, dim3(b->B), dim3(64), 0, b->stream, a, minus, d_x1, d_v, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}
int viekf_batch_boxplus(viekf_batch* b, const double* x, const double* dx, double* out, viekf_mem where) { return boxop(b, 0, x, dx, out, where); }
int viekf_batch_boxminus(viekf_batch* b, const double* x1, const double* x2, double* out, viekf_mem where) { return boxop(b, 1, x1, x2, out, where); }

int viekf_batch_eval_reset_jacobian(viekf_batch* b, const double* xm, double* xp, double* N, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!xm || (!xp && !N)) return fail(VIEKF_ERR_INVALID, "xm and at least one output must not be null");
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B;
  const double* d_xm = nullptr;
  double *d_xp = nullptr, *d_N = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(xm, B * b->nx, &d_xm), out(xp, B * b->nx, &d_xp), out(N, B * b->n * b->n, &d_N))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_eval_reset, dim3(b->B), dim3(256), 0, b->stream, a, d_xm, d_xp, d_N);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_get_cov_diag(viekf_batch* b, double* diag, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!diag) return fail(VIEKF_ERR_INVALID, "diag is null");
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = require_P(b, PForm::Lower)) return rc;
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(out(diag, (size_t)b->B * b->n, &d_o))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_cov_diag, dim3((b->n + 63) / 64, b->B), dim3(64), 0, b->stream, a, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_get_cov_block(viekf_batch* b, int32_t row0, int32_t col0, int32_t nrows, int32_t ncols, double* block,
                              viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!block) return fail(VIEKF_ERR_INVALID, "out is null");
  if (int rc = require_P(b, PForm::Full)) return rc;
  if (row0 < 0 || col0 < 0 || nrows < 1 || ncols < 1 || row0 + nrows > b->n || col0 + ncols > b->n)
    return fail(VIEKF_ERR_INVALID, "block outside the covariance");
  HIP_TRY(hipSetDevice(b->device));
  double* d_o = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(out(block, (size_t)b->B * nrows * ncols, &d_o))) return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_cov_block, dim3((nrows * ncols + 63) / 64, b->B), dim3(64), 0, b->stream, a, row0, col0, nrows, ncols, d_o);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_history_resize(viekf_batch* b, int32_t depth) {
  if (int rc = check_batch(b)) return rc;
  if (depth < 0 || depth > 4096) return fail(VIEKF_ERR_INVALID, "0 <= depth <= 4096");
  HIP_TRY(hipSetDevice(b->device));
  HIP_TRY(hipStreamSynchronize(b->stream));
  if (b->book.per_filter()) {       // every filter's live slot goes home
    if (int rc = gather_scatter_home(b, 1)) return rc;
    HIP_TRY(hipStreamSynchronize(b->stream));
  }
  if (b->book.live_slot() >= 0) {   // the live state lives in the ring: bring it home first, as it stands
    HIP_TRY(hipMemcpy(b->home_x, b->d_x, hist_nx(b), hipMemcpyDeviceToDevice));
    HIP_TRY(hipMemcpy(b->home_P, b->d_P, hist_nP(b), hipMemcpyDeviceToDevice));
  }
  b->book.resized(0);
  point_live(b);
  if (int rc = b->own.free(&b->h_x)) return rc;
  if (int rc = b->own.free(&b->h_P)) return rc;
  if (int rc = b->own.free(&b->h_len)) return rc;
  b->hist_depth = 0;
  if (depth == 0) return VIEKF_OK;
  if (int rc = b->own.alloc(&b->h_x, (size_t)depth * b->B * b->nxs)) return rc;
  if (int rc = b->own.alloc(&b->h_P, (size_t)depth * b->B * b->n * b->ld)) return rc;
  if (int rc = b->own.alloc(&b->h_len, (size_t)depth * b->B)) return rc;
  b->hist_depth = depth;
  b->book.resized(depth);
  return VIEKF_OK;
}

static int history_copy(viekf_batch* b, int32_t slot, bool save) {
  if (int rc = check_batch(b)) return rc;
  if (slot < 0 || slot >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "snapshot slot out of range (viekf_batch_history_resize first)");
  if (b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "whole-batch ring copies under per-filter live slots (viekf_batch_select_filters)");
  // (the covariance is copied as it stands, packed or not: the form travels with it)
  if (save) b->book.saved_to(slot); else b->book.restored_from(slot);
  HIP_TRY(hipSetDevice(b->device));
  struct State { double *x, *P; int* len; };
  const State live = {b->d_x, b->d_P, b->d_len}, ring = {slot_x(b, slot), slot_P(b, slot), b->h_len + (size_t)b->B * slot};
  const State &src = save ? live : ring, &dst = save ? ring : live;
  if (slot != b->book.live_slot()) {   // (the live state already IS this slot: only the feature counts move)
    HIP_TRY(hipMemcpyAsync(dst.x, src.x, hist_nx(b), hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(dst.P, src.P, hist_nP(b), hipMemcpyDeviceToDevice, b->stream));
  }
  HIP_TRY(hipMemcpyAsync(dst.len, src.len, sizeof(int) * (size_t)b->B, hipMemcpyDeviceToDevice, b->stream));
  return VIEKF_OK;
}
int viekf_batch_snapshot(viekf_batch* b, int32_t slot) { return history_copy(b, slot, true); }
int viekf_batch_restore(viekf_batch* b, int32_t slot) { return history_copy(b, slot, false); }

int viekf_batch_set_active(viekf_batch* b, const uint8_t* mask, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  HIP_TRY(hipSetDevice(b->device));
  if (!mask) { b->active_on = false; return VIEKF_OK; }
  if (!b->d_active)
    if (int rc = b->own.alloc(&b->d_active, (size_t)b->B)) return rc;
  const void* from = mask;
  if (where == VIEKF_HOST && b->async_host) {   // through the pinned ring: nothing to wait for (the mask itself stays a DEVICE copy:
    if (int rc = stage_begin(b, stage_size((size_t)b->B))) return rc;   // it outlives any number of launches)
    const size_t off = (b->pin_used + 255) & ~size_t(255);
    std::memcpy(b->h_pin + off, mask, (size_t)b->B);
    b->pin_used = off + (size_t)b->B;
    from = b->h_pin + off;
  }
  HIP_TRY(hipMemcpyAsync(b->d_active, from, (size_t)b->B, where == VIEKF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         b->stream));
  if (where == VIEKF_HOST && !b->async_host) HIP_TRY(hipStreamSynchronize(b->stream));   // (the caller's buffer may go away)
  b->active_on = true;
  return VIEKF_OK;
}

static int ring_filters(viekf_batch* b, const int32_t* slot, viekf_mem where, int to_ring) {
  if (int rc = check_batch(b)) return rc;
  if (!slot) return fail(VIEKF_ERR_INVALID, "slot is null");
  if (b->hist_depth <= 0) return fail(VIEKF_ERR_INVALID, "no history ring (viekf_batch_history_resize first)");
  if (b->book.live_slot() >= 0) return fail(VIEKF_ERR_INVALID, "per-filter ring copies need the live state in the batch's own buffers (viekf_batch_select(-1))");
  HIP_TRY(hipSetDevice(b->device));
  // (host slots are validated here; device slots by the kernel, which skips an out-of-range one and raises VIEKF_FLAG_INTERNAL)
  if (where == VIEKF_HOST)
    for (int i = 0; i < b->B; i++)
      if (slot[i] >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "ring slot out of range");
  if (int rc = canonicalize_all(b)) return rc;   // (single filters move between buffers: no buffer may end up of mixed form)
  if (!to_ring) b->book.filters_moved();
  const int* d_slot = nullptr;
  Staged st(b, where);
  if (where == VIEKF_HOST && !b->async_host) {   // (a buffer of the batch's own, not the staging region)
    if (!b->d_ringslot)
      if (int rc = b->own.alloc(&b->d_ringslot, (size_t)b->B)) return rc;
    HIP_TRY(hipMemcpyAsync(b->d_ringslot, slot, sizeof(int) * (size_t)b->B, hipMemcpyHostToDevice, b->stream));
    d_slot = b->d_ringslot;
  } else {   // (async: read by this one launch straight from the pinned ring, nothing to wait for)
    if (int rc = st.begin(in(slot, (size_t)b->B, &d_slot))) return rc;
  }
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_ring_copy, dim3(b->B), dim3(256), 0, b->stream, a, b->h_x, b->h_P, d_slot, to_ring, b->hist_depth);
  HIP_TRY(hipGetLastError());
  return st.finish(true);
}
int viekf_batch_snapshot_filters(viekf_batch* b, const int32_t* slot, viekf_mem where) { return ring_filters(b, slot, where, 1); }
int viekf_batch_restore_filters(viekf_batch* b, const int32_t* slot, viekf_mem where) { return ring_filters(b, slot, where, 0); }

int viekf_batch_select(viekf_batch* b, int32_t slot) {
  if (int rc = check_batch(b)) return rc;
  if (slot < -1 || slot >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "ring slot out of range (viekf_batch_history_resize first)");
  if (b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "viekf_batch_select under per-filter live slots (viekf_batch_select_filters)");
  b->book.select(slot);
  point_live(b);
  return VIEKF_OK;
}

int viekf_batch_propagate_to(viekf_batch* b, const double* u, const double* dt, int32_t dst_slot, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || !dt) return fail(VIEKF_ERR_INVALID, "u and dt must not be null");
  if (dst_slot < 0 || dst_slot >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "ring slot out of range (viekf_batch_history_resize first)");
  if (b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "viekf_batch_propagate_to under per-filter live slots (viekf_batch_propagate_filters_to)");
  if (dst_slot == b->book.live_slot()) return viekf_batch_propagate(b, u, dt, where);
  // (a filter outside a participation mask would have nothing written into the destination slot, which then becomes the live
  //  state: the zero-copy ring is for filters that advance together)
  if (b->active_on) return fail(VIEKF_ERR_INVALID, "viekf_batch_propagate_to under a participation mask (viekf_batch_set_active(NULL) first)");
  HIP_TRY(hipSetDevice(b->device));
  const double *d_u = nullptr, *d_dt = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(u, (size_t)6 * b->B, &d_u), in(dt, (size_t)b->B, &d_dt))) return rc;
  if (use_resident(b)) {   // the fused kernel loads P from the live slot and stores it into the destination: no copy at all
    if (int rc = launch_resident(b, true, d_u, d_dt, nullptr, nullptr, 0, nullptr, 0, nullptr, dst_slot))
      return rc;
    if (int rc = viekf_batch_select(b, dst_slot)) return rc;
  } else {                 // streaming family works in place: copy, then propagate the copy
    HIP_TRY(hipMemcpyAsync(slot_x(b, dst_slot), b->d_x, hist_nx(b), hipMemcpyDeviceToDevice, b->stream));
    HIP_TRY(hipMemcpyAsync(slot_P(b, dst_slot), b->d_P, hist_nP(b), hipMemcpyDeviceToDevice, b->stream));
    b->book.saved_to(dst_slot);
    if (int rc = viekf_batch_select(b, dst_slot)) return rc;
    if (int rc = launch_propagate(b, d_u, d_dt)) return rc;
  }
  return st.finish(true);
}

int viekf_batch_propagate_n_to(viekf_batch* b, int32_t K, const double* u, const double* dt, const int32_t* dst_slots,
                               int32_t* intermediates_written, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || !dt || !dst_slots) return fail(VIEKF_ERR_INVALID, "u, dt and dst_slots must not be null");
  if (K < 1 || K > 64) return fail(VIEKF_ERR_INVALID, "1 <= K <= 64 propagates per call");
  if (b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "viekf_batch_propagate_n_to under per-filter live slots");
  for (int k = 0; k < K; k++) {
    if (dst_slots[k] < 0 || dst_slots[k] >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "ring slot out of range (viekf_batch_history_resize first)");
    if (dst_slots[k] == b->book.live_slot()) return fail(VIEKF_ERR_INVALID, "a destination slot is the live slot");
    for (int j = 0; j < k; j++)
      if (dst_slots[j] == dst_slots[k]) return fail(VIEKF_ERR_INVALID, "destination slots must differ");
  }
  if (intermediates_written) *intermediates_written = 1;
  if (K == 1 || !use_resident(b) || b->active_on) {   // one slot at a time, every slot written
    for (int k = 0; k < K; k++)
      if (int rc = viekf_batch_propagate_to(b, u + (size_t)6 * b->B * k, dt + (size_t)b->B * k, dst_slots[k], where)) return rc;
    return VIEKF_OK;
  }
  HIP_TRY(hipSetDevice(b->device));
  const double *d_u = nullptr, *d_dt = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(u, (size_t)6 * b->B * K, &d_u), in(dt, (size_t)b->B * K, &d_dt))) return rc;
  const int last = dst_slots[K - 1];
  // ONE launch of the fused kernel: P is loaded from the live slot, stays on chip through the K propagates and is stored into the
  // last slot only
  if (int rc = launch_resident(b, true, d_u, d_dt, nullptr, nullptr, 0, nullptr, 0, nullptr, last, K)) return rc;
  if (int rc = viekf_batch_select(b, last)) return rc;
  if (intermediates_written) *intermediates_written = 0;
  return st.finish(true);
}

int viekf_batch_select_filters(viekf_batch* b, const int32_t* slot) {
  if (int rc = check_batch(b)) return rc;
  if (!slot) return fail(VIEKF_ERR_INVALID, "slot is null");
  if (b->hist_depth <= 0) return fail(VIEKF_ERR_INVALID, "no history ring (viekf_batch_history_resize first)");
  if (b->book.live_slot() >= 0) return fail(VIEKF_ERR_INVALID, "per-filter live slots need the live state in the batch's own buffers (viekf_batch_select(-1))");
  for (int i = 0; i < b->B; i++) {
    if (slot[i] >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "ring slot out of range");
    if (slot[i] < 0 && !b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "the first call has to name a slot for every filter");
  }
  HIP_TRY(hipSetDevice(b->device));
  if (int rc = canonicalize_all(b)) return rc;   // (per-filter live slots keep today's canonical path: every buffer first)
  if (!b->book.per_filter()) {
    if (!b->d_smap)
      if (int rc = b->own.alloc(&b->d_smap, (size_t)b->B)) return rc;
    b->live_slots.assign((size_t)b->B, 0);
    b->book.enter_per_filter();
    point_live(b);
  }
  for (int i = 0; i < b->B; i++)
    if (slot[i] >= 0) b->live_slots[(size_t)i] = slot[i];
  // the device's copy of the map follows in stream order (a launch of one small kernel, not a copy command between two kernels)
  const int32_t* d_slot = nullptr;
  Staged st(b, VIEKF_HOST);
  if (int rc = st.begin(in(slot, (size_t)b->B, &d_slot))) return rc;
  hipLaunchKernelGGL(k_set_smap, dim3((unsigned)((b->B + 255) / 256)), dim3(256), 0, b->stream, b->d_smap, d_slot, b->B);
  HIP_TRY(hipGetLastError());
  if (int rc = st.finish(true)) return rc;
  b->book.filters_moved();
  return VIEKF_OK;
}

// The one masked launch behind both per-filter propagate entry points (which have checked every argument): filter i with
// dst_slot[i] >= 0 -- and k_count[i] > 0 where counts are given -- goes from its live slot into dst_slot[i], by k_count[i]
// propagates (one without counts; counts are for the fused family only); every other filter is outside the launch's own mask.
// u / dt hold Kstaged propagates per filter, kmax is the most any filter takes.
static int propagate_filters_masked(viekf_batch* b, const double* u, const double* dt, int Kstaged, int kmax, const int32_t* k_count,
                                    const int32_t* dst_slot, viekf_mem where) {
  const size_t B = (size_t)b->B;
  // the participation mask and the destination map of THIS launch, through the pinned staging like the other per-call arguments
  std::vector<unsigned char> act(B);
  std::vector<int32_t> omap(B), kc(k_count ? B : 0);
  for (size_t i = 0; i < B; i++) {
    const bool on = dst_slot[i] >= 0 && (!k_count || k_count[i] > 0);
    act[i] = on ? 1 : 0;
    omap[i] = (on ? dst_slot[i] : b->live_slots[i]) * b->B + (int32_t)i;
    if (k_count) kc[i] = on ? k_count[i] : 1;   // (a filter outside the mask never reads it)
  }
  const bool in_place = !use_resident(b);   // (the HBM-path family: it needs the destination slots themselves instead of counts)
  const double *d_u = nullptr, *d_dt = nullptr;
  const unsigned char* d_act = nullptr;
  const int32_t *d_omap = nullptr, *d_extra = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(u, 6 * B * (size_t)Kstaged, &d_u), in(dt, B * (size_t)Kstaged, &d_dt), in_host(act.data(), B, &d_act),
                        in_host(omap.data(), B, &d_omap), in_host(in_place ? dst_slot : (k_count ? kc.data() : nullptr), B, &d_extra)))
    return rc;
  if (!in_place) {   // the fused kernel loads filter b from its live slot and stores it into dst_slot[b]: no copy at all
    if (int rc = launch_resident(b, true, d_u, d_dt, nullptr, nullptr, 0, nullptr, 0, nullptr, -1, kmax, d_omap, k_count ? d_extra : nullptr, d_act))
      return rc;
  } else {           // the HBM-path family works in place: copy slot -> slot, then propagate the copy
    StreamArgs a = make_args(b, d_act);
    hipLaunchKernelGGL(k_ring_copy, dim3(b->B), dim3(256), 0, b->stream, a, b->h_x, b->h_P, d_extra, 1, b->hist_depth);
    if (hipGetLastError() != hipSuccess) return fail(VIEKF_ERR_HIP, "k_ring_copy launch failed");
  }
  for (size_t i = 0; i < B; i++)   // (the fused kernel moves the device's map entries itself)
    if (act[i]) b->live_slots[i] = dst_slot[i];
  if (in_place) {
    hipLaunchKernelGGL(k_set_smap, dim3((unsigned)((b->B + 255) / 256)), dim3(256), 0, b->stream, b->d_smap, d_extra, b->B);
    if (hipGetLastError() != hipSuccess) return fail(VIEKF_ERR_HIP, "k_set_smap launch failed");
    if (int rc = launch_propagate(b, d_u, d_dt, d_act)) return rc;
  }
  return st.finish(true);
}

int viekf_batch_propagate_filters_to(viekf_batch* b, const double* u, const double* dt, const int32_t* dst_slot, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || !dt || !dst_slot) return fail(VIEKF_ERR_INVALID, "u, dt and dst_slot must not be null");
  if (!b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "viekf_batch_select_filters first");
  // (the launch runs under a mask of its own, dst_slot[b] >= 0: a caller's mask would be ignored and a filter it masked out
  //  stepped anyway -- refused like viekf_batch_propagate_to)
  if (b->active_on)
    return fail(VIEKF_ERR_INVALID, "viekf_batch_propagate_filters_to under a participation mask (viekf_batch_set_active(NULL) first; dst_slot < 0 skips a filter)");
  bool any = false;
  for (int i = 0; i < b->B; i++) {
    if (dst_slot[i] >= b->hist_depth) return fail(VIEKF_ERR_INVALID, "ring slot out of range");
    if (dst_slot[i] >= 0 && dst_slot[i] == b->live_slots[(size_t)i]) return fail(VIEKF_ERR_INVALID, "a destination slot is the filter's live slot");
    any |= dst_slot[i] >= 0;
  }
  if (!any) return VIEKF_OK;
  HIP_TRY(hipSetDevice(b->device));
  return propagate_filters_masked(b, u, dt, 1, 1, nullptr, dst_slot, where);
}

int viekf_batch_propagate_n_filters_to(viekf_batch* b, int32_t Kmax, const double* u, const double* dt, const int32_t* k_count,
                                       const int32_t* dst_slot, int32_t* intermediates_written, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (!u || !dt || !k_count || !dst_slot) return fail(VIEKF_ERR_INVALID, "u, dt, k_count and dst_slot must not be null");
  if (Kmax < 1 || Kmax > 64) return fail(VIEKF_ERR_INVALID, "1 <= Kmax <= 64 propagates per call");
  if (!b->book.per_filter()) return fail(VIEKF_ERR_INVALID, "viekf_batch_select_filters first");
  if (b->active_on)   // (the call runs under a mask of its own, like viekf_batch_propagate_filters_to)
    return fail(VIEKF_ERR_INVALID, "viekf_batch_propagate_n_filters_to under a participation mask (viekf_batch_set_active(NULL) first; k_count 0 or dst_slot < 0 skips a filter)");
  const size_t B = (size_t)b->B;
  const int H = b->hist_depth;
  // every check before anything changes: the steps below cannot be refused half way
  int kmax = 0;
  for (size_t i = 0; i < B; i++) {
    if (k_count[i] < 0 || k_count[i] > Kmax) return fail(VIEKF_ERR_INVALID, "need 0 <= k_count[b] <= Kmax");
    if (dst_slot[i] >= H) return fail(VIEKF_ERR_INVALID, "ring slot out of range");
    if (k_count[i] == 0 || dst_slot[i] < 0) continue;
    if (dst_slot[i] == b->live_slots[i]) return fail(VIEKF_ERR_INVALID, "a destination slot is the filter's live slot");
    kmax = std::max(kmax, (int)k_count[i]);
  }
  if (kmax >= 2 && H < 3)   // (live slot, destination and the scratch slot of the step-by-step route: whichever route is taken)
    return fail(VIEKF_ERR_INVALID, "several propagates per filter need a ring of at least 3 slots");
  if (intermediates_written) *intermediates_written = 0;
  if (kmax == 0) return VIEKF_OK;
  HIP_TRY(hipSetDevice(b->device));
  // ONE launch of the fused kernel's multi-propagate instance: filter b is loaded from its live slot, P stays on chip through its
  // own k_count[b] propagates and is stored into dst_slot[b] only
  if (kmax >= 2 && use_resident(b) && !use_tiles(b)) return propagate_filters_masked(b, u, dt, Kmax, kmax, k_count, dst_slot, where);
  // Step by step (the HBM-path family, the tile family, one propagate per filter): step k of filter b goes into dst_slot[b] or
  // into its scratch slot -- the slot after dst_slot[b] in ring order that is not its live slot -- by turns, the last one into
  // dst_slot[b].  (viekf_batch_propagate_filters_to moves the host's live-slot mirror after each step it has issued.)
  std::vector<int32_t> step(B), scratch(B, -1);
  for (size_t i = 0; i < B; i++) {   // (fixed by the slot the filter starts from)
    if (dst_slot[i] < 0 || k_count[i] < 2) continue;
    scratch[i] = (dst_slot[i] + 1) % H;
    if (scratch[i] == b->live_slots[i]) scratch[i] = (scratch[i] + 1) % H;
  }
  for (int k = 0; k < kmax; k++) {
    for (size_t i = 0; i < B; i++) {
      step[i] = -1;
      if (dst_slot[i] < 0 || k >= k_count[i]) continue;
      step[i] = ((k_count[i] - 1 - k) & 1) ? scratch[i] : dst_slot[i];
    }
    if (int rc = viekf_batch_propagate_filters_to(b, u + 6 * B * (size_t)k, dt + B * (size_t)k, step.data(), where)) return rc;
    if (k + 1 < kmax && intermediates_written) *intermediates_written = 1;
  }
  return VIEKF_OK;
}

int viekf_batch_update(viekf_batch* b, int32_t type, const double* z, int32_t zdim, const double* R, int32_t rdim,
                       int32_t r_mode, const int32_t* slot, const uint8_t* active, int32_t* result, viekf_mem where) {
  if (int rc = check_batch(b)) return rc;
  if (int rc = require_P(b, PForm::Full)) return rc;
  if (!z || !R) return fail(VIEKF_ERR_INVALID, "z and R must not be null");
  if (type < 0 || type >= VIEKF_TOTAL_MEAS || type == VIEKF_PIXEL_VEL)
    return fail(VIEKF_ERR_UNSUPPORTED, "measurement type not supported (PIXEL_VEL is an empty TODO in the reference)");
  if (zdim < 1 || zdim > 4 || rdim < 1 || rdim > 3 || r_mode < 0 || r_mode > 1)
    return fail(VIEKF_ERR_INVALID, "need 1 <= zdim <= 4, 1 <= rdim <= 3, r_mode 0 or 1");
  const bool needs_slot = type == VIEKF_QZETA || type == VIEKF_FEAT || type == VIEKF_DEPTH || type == VIEKF_INV_DEPTH;
  if (needs_slot && !slot) return fail(VIEKF_ERR_INVALID, "slot must not be null for feature measurements");
  HIP_TRY(hipSetDevice(b->device));
  const size_t B = (size_t)b->B, rr = (size_t)rdim * rdim;
  const double *d_z = nullptr, *d_R = nullptr;
  const int32_t* d_slot = nullptr;
  const uint8_t* d_act = nullptr;
  int32_t* d_res = nullptr;
  Staged st(b, where);
  if (int rc = st.begin(in(z, B * zdim, &d_z), in(R, r_mode ? B * rr : rr, &d_R), in(slot, B, &d_slot), in(active, B, &d_act),
                        out(result, B, &d_res)))
    return rc;
  StreamArgs a = make_args(b);
  hipLaunchKernelGGL(k_update_generic<kThreads>, dim3(b->B), dim3(kThreads), GenLds(b->nxs, b->n).bytes(), b->stream, a, type, zdim,
                     rdim, d_z, d_slot, d_R, r_mode ? (long)rr : 0L, d_act, d_res);
  HIP_TRY(hipGetLastError());
  return st.finish();
}

int viekf_batch_update_feat(viekf_batch* b, const double* z, const int32_t* slot, int32_t M, const double* R,
                            int32_t r_mode, int32_t* result, viekf_mem where) {
  return update_or_step(b, nullptr, nullptr, false, z, slot, M, R, r_mode, result, where);
}

int viekf_batch_step(viekf_batch* b, const double* u, const double* dt, const double* z, const int32_t* slot,
                     int32_t M, const double* R, int32_t r_mode, int32_t* result, viekf_mem where) {
  return update_or_step(b, u, dt, true, z, slot, M, R, r_mode, result, where);
}

int viekf_batch_step_n(viekf_batch* b, int32_t K, const double* u, const double* dt, const double* z, const int32_t* slot,
                       int32_t M, const double* R, int32_t r_mode, int32_t* result, viekf_mem where) {
  return update_or_step(b, u, dt, true, z, slot, M, R, r_mode, result, where, K);
}

}  // extern "C"

// the companions of a batch, each with its handle and helpers (still this one translation unit)
#include "viekf_capi_body.hpp"
#include "viekf_capi_diag.hpp"
#include "viekf_capi_frame.hpp"
#include "viekf_capi_depth.hpp"
#include "viekf_capi_pixvel.hpp"
#include "viekf_capi_node.hpp"
#include "viekf_capi_map.hpp"
#include "viekf_capi_rec.hpp"
