// viekf_cam.hip -- the device-resident camera model behind include/viekf_cam.h: radial-tangential lens distortion for
// `batch` cameras.  The header states the model operation by operation; every formula below restates one
// of its lines in double, in its order of operations (this file is compiled without FMA contraction, like the tracker
// and the simulator), and tests/cam_ref.py restates them once more in numpy.
//
//   k_cam_distort     one lane per (camera, point): the forward model and its Jacobian
//   k_cam_undistort   one lane per (camera, point): Newton on the forward model, R_out = J_u R J_u^T, the status
//   k_cam_mask        tiles x sets, four horizontally adjacent pixels per thread: 255 where the raw pixel inverts
//   k_cam_warp<DIR>   tiles x batch, four pixels per thread: map the output pixel, gather src bilinearly, depth nearest
//
// The Newton loop is divergent per lane; a wave leaves it when all its lanes are done.  No LDS, no atomics, no
// synchronisation between lanes: a result depends on its own inputs and its camera's intrinsics row only.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/viekf_cam.h"
#include "viekf_hostkit.hpp"

namespace {

constexpr int kTileW = 64, kTileH = 16;           // pixel kernels: 16 x 16 threads, four pixels each along x
constexpr int kRow = 16;                          // doubles per intrinsics row in device memory (128 bytes)
// row: f0 f1 c0 c1 | k1 k2 p1 p2 | F0 F1 C0 C1 | min_det r_valid^2 r_valid 0

struct Cam { double f0, f1, c0, c1, k1, k2, p1, p2, F0, F1, C0, C1, md, rv2; };
struct Fwd { double xd, yd, j00, j01, j11, det; bool in; };

#define CD __host__ __device__ __forceinline__
#define SD __device__ __forceinline__

// forward(x, y) of the header; J10 = J01
CD void forward(const Cam& k, double x, double y, Fwd& o) {
  const double r2 = x * x + y * y;
  const double rad = 1.0 + k.k1 * r2 + k.k2 * r2 * r2;
  const double drad = k.k1 + 2.0 * k.k2 * r2;
  o.xd = x * rad + 2.0 * k.p1 * x * y + k.p2 * (r2 + 2.0 * x * x);
  o.yd = y * rad + k.p1 * (r2 + 2.0 * y * y) + 2.0 * k.p2 * x * y;
  o.j00 = rad + 2.0 * x * x * drad + 2.0 * k.p1 * y + 6.0 * k.p2 * x;
  o.j01 = 2.0 * x * y * drad + 2.0 * k.p1 * x + 2.0 * k.p2 * y;
  o.j11 = rad + 2.0 * y * y * drad + 6.0 * k.p1 * y + 2.0 * k.p2 * x;
  o.det = o.j00 * o.j11 - o.j01 * o.j01;
  o.in = r2 <= k.rv2 && o.det > k.md;             // (a NaN is not inside)
}

SD Cam load_cam(const double* __restrict__ row) {
  Cam k;
  k.f0 = row[0]; k.f1 = row[1]; k.c0 = row[2]; k.c1 = row[3];
  k.k1 = row[4]; k.k2 = row[5]; k.p1 = row[6]; k.p2 = row[7];
  k.F0 = row[8]; k.F1 = row[9]; k.C0 = row[10]; k.C1 = row[11];
  k.md = row[12]; k.rv2 = row[13];
  return k;
}

// undistort of the header for the raw pixel (u, v): the status; on VIEKF_CAM_OK the ideal pixel and J_u = [j00 j01; j10 j11]
SD int undistort(const Cam& k, double u, double v, double* zi, double* ju) {
  if (u != u || v != v) return VIEKF_CAM_PADDING;
  const double xd = (u - k.c0) / k.f0, yd = (v - k.c1) / k.f1;
  double x = xd, y = yd;
  Fwd F;
  bool stopped = false;
  for (int it = 0; it < VIEKF_CAM_MAX_ITER; it++) {
    forward(k, x, y, F);
    if (!F.in) return VIEKF_CAM_OUT_OF_MODEL;
    const double ex = xd - F.xd, ey = yd - F.yd;
    const double sx = (F.j11 * ex - F.j01 * ey) / F.det, sy = (F.j00 * ey - F.j01 * ex) / F.det;
    x = x + sx;
    y = y + sy;
    if (sx * sx + sy * sy <= VIEKF_CAM_STEP_TOL * VIEKF_CAM_STEP_TOL) { stopped = true; break; }
  }
  if (!stopped) return VIEKF_CAM_OUT_OF_MODEL;
  forward(k, x, y, F);
  if (!F.in) return VIEKF_CAM_OUT_OF_MODEL;
  zi[0] = k.F0 * x + k.C0;
  zi[1] = k.F1 * y + k.C1;
  if (ju) {
    ju[0] = k.F0 * F.j11 / F.det / k.f0;
    ju[1] = -k.F0 * F.j01 / F.det / k.f1;
    ju[2] = -k.F1 * F.j01 / F.det / k.f0;
    ju[3] = k.F1 * F.j00 / F.det / k.f1;
  }
  return VIEKF_CAM_OK;
}

// ---- points ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_cam_distort(const double* __restrict__ K, int per, int B, int M,
                                                     const double* __restrict__ zi, double* __restrict__ zr, double* __restrict__ J) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * M) return;
  const int b = (int)(i / M);
  const Cam k = load_cam(K + (per ? (long long)b * kRow : 0ll));
  const double u = zi[2 * i], v = zi[2 * i + 1];
  const double x = (u - k.C0) / k.F0, y = (v - k.C1) / k.F1;
  Fwd F;
  forward(k, x, y, F);
  zr[2 * i] = k.f0 * F.xd + k.c0;
  zr[2 * i + 1] = k.f1 * F.yd + k.c1;
  if (J) {                                        // column-major d raw / d ideal
    J[4 * i] = k.f0 * F.j00 / k.F0;
    J[4 * i + 1] = k.f1 * F.j01 / k.F0;
    J[4 * i + 2] = k.f0 * F.j01 / k.F1;
    J[4 * i + 3] = k.f1 * F.j11 / k.F1;
  }
}

__global__ __launch_bounds__(256) void k_cam_undistort(const double* __restrict__ K, int per, int B, int M,
                                                       const double* __restrict__ zr, const double* __restrict__ R, int r_mode,
                                                       double* __restrict__ zi, double* __restrict__ Ro, int* __restrict__ status) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)B * M) return;
  const int b = (int)(i / M);
  const Cam k = load_cam(K + (per ? (long long)b * kRow : 0ll));
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double z[2] = {nan, nan}, ju[4];
  const int st = undistort(k, zr[2 * i], zr[2 * i + 1], z, ju);
  zi[2 * i] = z[0];
  zi[2 * i + 1] = z[1];
  if (status) status[i] = st;
  if (Ro) {
    const double* r = R + (r_mode == 0 ? 0ll : (r_mode == 1 ? 4ll * b : 4ll * i));
    const double r00 = r[0], r10 = r[1], r01 = r[2], r11 = r[3];
    double o00 = r00, o10 = r10, o01 = r01, o11 = r11;
    if (st == VIEKF_CAM_OK) {
      const double t00 = ju[0] * r00 + ju[1] * r10, t01 = ju[0] * r01 + ju[1] * r11;
      const double t10 = ju[2] * r00 + ju[3] * r10, t11 = ju[2] * r01 + ju[3] * r11;
      o00 = t00 * ju[0] + t01 * ju[1];
      o10 = t10 * ju[0] + t11 * ju[1];
      o11 = t10 * ju[2] + t11 * ju[3];
      o01 = o10;                                  // (symmetric by construction: the off-diagonal is computed once)
    }
    Ro[4 * i] = o00; Ro[4 * i + 1] = o10; Ro[4 * i + 2] = o01; Ro[4 * i + 3] = o11;
  }
}

// ---- pixels ----------------------------------------------------------------------------------------------------------------
// four grey bytes and (dmm != null) four depths of the pixels x0 .. x0 + 3 of row `a`: whole groups where W % 4 == 0, pairs
// otherwise (W is even: every row starts on a pair and a pair is inside or outside), as k_sim_render stores them
SD void store4(uint8_t* __restrict__ img, float* __restrict__ dmm, long long a, int x0, int W, const unsigned* q, const float* m) {
  if ((W & 3) == 0) {
    *reinterpret_cast<unsigned*>(img + a) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    if (dmm) *reinterpret_cast<float4*>(dmm + a) = make_float4(m[0], m[1], m[2], m[3]);
  } else {
    *reinterpret_cast<unsigned short*>(img + a) = (unsigned short)(q[0] | (q[1] << 8));
    if (dmm) *reinterpret_cast<float2*>(dmm + a) = make_float2(m[0], m[1]);
    if (x0 + 2 < W) {
      *reinterpret_cast<unsigned short*>(img + a + 2) = (unsigned short)(q[2] | (q[3] << 8));
      if (dmm) *reinterpret_cast<float2*>(dmm + a + 2) = make_float2(m[2], m[3]);
    }
  }
}

__global__ __launch_bounds__(256) void k_cam_mask(const double* __restrict__ K, int W, int H, int tiles_x, uint8_t* __restrict__ mask) {
  const int s = blockIdx.y, tid = threadIdx.x;
  const Cam k = load_cam(K + (long long)s * kRow);
  const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const int x0 = tile_x * kTileW + (tid & 15) * 4, y = tile_y * kTileH + (tid >> 4);
  if (y >= H || x0 >= W) return;
  unsigned q[4];
  float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double z[2];
    q[i] = 0u;
    if (x0 + i < W) q[i] = undistort(k, (double)(x0 + i), (double)y, z, nullptr) == VIEKF_CAM_OK ? 255u : 0u;
  }
  store4(mask, nullptr, ((long long)s * H + y) * W + x0, x0, W, q, m);
}

// src at (sx, sy) of the header: grey bilinear in double over the four neighbours, depth nearest
SD void sample(const uint8_t* __restrict__ src, const float* __restrict__ sd, int W, int H, double sx, double sy, unsigned fill,
               unsigned* g, float* mm) {
  *g = fill;
  *mm = __int_as_float(0x7f800000);
  if (!(sx >= 0.0 && sx <= (double)(W - 1) && sy >= 0.0 && sy <= (double)(H - 1))) return;   // (a NaN leaves here too)
  const double fx = floor(sx), fy = floor(sy);
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
  const double ax = sx - fx, ay = sy - fy;
  const double i00 = (double)src[(long long)y0 * W + x0], i01 = (double)src[(long long)y0 * W + x1];
  const double i10 = (double)src[(long long)y1 * W + x0], i11 = (double)src[(long long)y1 * W + x1];
  const double v = (1.0 - ay) * ((1.0 - ax) * i00 + ax * i01) + ay * ((1.0 - ax) * i10 + ax * i11);
  *g = (unsigned)floor(v + 0.5);
  if (sd) {
    const int xn = (int)floor(sx + 0.5), yn = (int)floor(sy + 0.5);      // (<= W - 1, H - 1: sx <= W - 1, sy <= H - 1)
    *mm = sd[(long long)yn * W + xn];
  }
}

template <int DIR>
__global__ __launch_bounds__(256) void k_cam_warp(const double* __restrict__ K, int per, int W, int H, int tiles_x, unsigned fill,
                                                  const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                  const float* __restrict__ sdep, float* __restrict__ ddep) {
  const int b = blockIdx.y, tid = threadIdx.x;
  const Cam k = load_cam(K + (per ? (long long)b * kRow : 0ll));
  const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const int x0 = tile_x * kTileW + (tid & 15) * 4, y = tile_y * kTileH + (tid >> 4);
  if (y >= H || x0 >= W) return;
  const long long img0 = (long long)b * H * W;
  const uint8_t* s8 = src + img0;
  const float* sd = sdep ? sdep + img0 : nullptr;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  unsigned q[4];
  float m[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    q[i] = fill;
    m[i] = __int_as_float(0x7f800000);
    if (x0 + i < W) {
      double sx = nan, sy = nan;                  // (a pixel outside the model samples nowhere)
      if (DIR == VIEKF_CAM_RECTIFY) {
        Fwd F;
        forward(k, ((double)(x0 + i) - k.C0) / k.F0, ((double)y - k.C1) / k.F1, F);
        if (F.in) { sx = k.f0 * F.xd + k.c0; sy = k.f1 * F.yd + k.c1; }
      } else {
        double z[2];
        if (undistort(k, (double)(x0 + i), (double)y, z, nullptr) == VIEKF_CAM_OK) { sx = z[0]; sy = z[1]; }
      }
      sample(s8, sd, W, H, sx, sy, fill, &q[i], &m[i]);
    }
  }
  store4(dst, ddep, img0 + (long long)y * W + x0, x0, W, q, m);
}

}  // namespace

struct viekf_cam {
  int B = 0, sets = 1, device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevOwner own;                                   // every device buffer below
  double* K = nullptr;                            // [batch][kRow]; row 0 alone is read while one set is shared
  std::vector<viekf_cam_intrinsics> k;            // the sets as given, [sets]
  std::vector<double> r_valid;                    // [sets]
  // growable device staging for callers with host pointers (bytes)
  char* stage[4] = {nullptr, nullptr, nullptr, nullptr};
  size_t stage_sz[4] = {0, 0, 0, 0};
};

namespace {

void cam_delete(viekf_cam* c) {
  c->own.release_all();
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

template <class T>
int cam_stage(viekf_cam* c, int i, size_t bytes, T** out) {
  if (int rc = c->own.reserve(&c->stage[i], &c->stage_sz[i], bytes, c->stream)) return rc;
  *out = reinterpret_cast<T*>(c->stage[i]);
  return VIEKF_OK;
}

int set_dev(const viekf_cam* c) {
  HIP_TRY(hipSetDevice(c->device));
  return VIEKF_OK;
}

Cam host_cam(const viekf_cam_intrinsics& k, double r_valid) {
  Cam c;
  c.f0 = k.focal[0]; c.f1 = k.focal[1]; c.c0 = k.center[0]; c.c1 = k.center[1];
  c.k1 = k.dist[0]; c.k2 = k.dist[1]; c.p1 = k.dist[2]; c.p2 = k.dist[3];
  c.F0 = k.out_focal[0]; c.F1 = k.out_focal[1]; c.C0 = k.out_center[0]; c.C1 = k.out_center[1];
  c.md = k.min_det; c.rv2 = r_valid * r_valid;
  return c;
}

// the polar scan of the header: the largest scanned radius up to which every sample has det > min_det
double derive_r_valid(const viekf_cam_intrinsics& k) {
  const Cam c = host_cam(k, VIEKF_CAM_SCAN_CAP);
  const int rings = (int)(VIEKF_CAM_SCAN_CAP / VIEKF_CAM_SCAN_STEP);
  double rv = 0.0;
  for (int i = 1; i <= rings; i++) {
    const double r = i * VIEKF_CAM_SCAN_STEP;
    for (int j = 0; j < VIEKF_CAM_SCAN_DIRS; j++) {
      const double th = 2.0 * M_PI * j / VIEKF_CAM_SCAN_DIRS;
      Fwd F;
      forward(c, r * std::cos(th), r * std::sin(th), F);
      if (!(F.det > k.min_det)) return rv;
    }
    rv = r;
  }
  return rv;
}

int check_intrinsics(const viekf_cam_intrinsics& k) {
  const double* v = reinterpret_cast<const double*>(&k);
  for (size_t i = 0; i < sizeof(k) / sizeof(double); i++)
    if (!std::isfinite(v[i])) return fail(VIEKF_ERR_INVALID, "every field of viekf_cam_intrinsics must be finite");
  if (!(k.focal[0] > 0.0) || !(k.focal[1] > 0.0) || !(k.out_focal[0] > 0.0) || !(k.out_focal[1] > 0.0))
    return fail(VIEKF_ERR_INVALID, "focal and out_focal must be > 0");
  return VIEKF_OK;
}

// derive r_valid for every set, fill the device table (the caller has set the device)
int upload_sets(viekf_cam* c, const viekf_cam_intrinsics* k, int sets) {
  std::vector<double> rows((size_t)sets * kRow, 0.0), rv((size_t)sets);
  for (int s = 0; s < sets; s++) {
    if (int rc = check_intrinsics(k[s])) return rc;
    rv[s] = derive_r_valid(k[s]);
    double* r = rows.data() + (size_t)s * kRow;
    r[0] = k[s].focal[0]; r[1] = k[s].focal[1]; r[2] = k[s].center[0]; r[3] = k[s].center[1];
    for (int i = 0; i < 4; i++) r[4 + i] = k[s].dist[i];
    r[8] = k[s].out_focal[0]; r[9] = k[s].out_focal[1]; r[10] = k[s].out_center[0]; r[11] = k[s].out_center[1];
    r[12] = k[s].min_det; r[13] = rv[s] * rv[s]; r[14] = rv[s];
  }
  HIP_TRY(hipStreamSynchronize(c->stream));       // (queued work may still read the table)
  HIP_TRY(hipMemcpy(c->K, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice));
  c->k.assign(k, k + sets);
  c->r_valid = rv;
  c->sets = sets;
  return VIEKF_OK;
}

int check_image(int32_t width, int32_t height) {
  if (width < 4 || height < 4 || width > 16384 || height > 16384) return fail(VIEKF_ERR_INVALID, "width and height must be in [4, 16384]");
  if (width & 1) return fail(VIEKF_ERR_INVALID, "width must be even: pixels are stored in pairs (in groups of four when width % 4 == 0)");
  return VIEKF_OK;
}

bool misaligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" {

int viekf_cam_intrinsics_default(viekf_cam_intrinsics* k) {
  if (!k) return fail(VIEKF_ERR_INVALID, "intrinsics is null");
  std::memset(k, 0, sizeof(*k));
  k->focal[0] = k->focal[1] = 1.0;
  k->out_focal[0] = k->out_focal[1] = 1.0;
  return VIEKF_OK;
}

int viekf_cam_load_yaml(const char* path, const char* params_path, viekf_cam_intrinsics* out) {
  if (!path || !out) return fail(VIEKF_ERR_INVALID, "null argument");
  viekf_cam_intrinsics k;
  viekf_cam_intrinsics_default(&k);
  viekf::YamlMap m;
  std::string err;
  if (!viekf::yaml_parse_file(path, m, err)) return fail(VIEKF_ERR_YAML, err);
  if (!viekf::yaml_get_doubles(m, "cam_center", k.center, 2, err) || !viekf::yaml_get_doubles(m, "focal_len", k.focal, 2, err))
    return fail(VIEKF_ERR_YAML, std::string(path) + ": " + err);
  if (m.count("distortion") && !viekf::yaml_get_doubles(m, "distortion", k.dist, 4, err)) return fail(VIEKF_ERR_YAML, std::string(path) + ": " + err);
  for (int i = 0; i < 2; i++) { k.out_focal[i] = k.focal[i]; k.out_center[i] = k.center[i]; }
  if (params_path) {
    viekf::YamlMap pm;
    if (!viekf::yaml_parse_file(params_path, pm, err)) return fail(VIEKF_ERR_YAML, err);
    if (!viekf::yaml_get_doubles(pm, "cam_center", k.out_center, 2, err) || !viekf::yaml_get_doubles(pm, "focal_len", k.out_focal, 2, err))
      return fail(VIEKF_ERR_YAML, std::string(params_path) + ": " + err);
  }
  *out = k;
  return VIEKF_OK;
}

int viekf_cam_create(int32_t batch, int32_t device, viekf_cam** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "out is null");
  *out = nullptr;
  if (batch <= 0 || batch > 65535) return fail(VIEKF_ERR_INVALID, "batch must be in [1, 65535]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(VIEKF_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  }
  if (device < 0 || device >= ndev) return fail(VIEKF_ERR_NO_DEVICE, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  viekf_cam* c = new (std::nothrow) viekf_cam();
  if (!c) return fail(VIEKF_ERR_HIP, "out of host memory");
  c->B = batch;
  c->device = device;
  auto fin = [&](int code) { cam_delete(c); return code; };
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return fin(fail(VIEKF_ERR_HIP, "hipStreamCreate failed"));
  c->own_stream = true;
  if (int rc = c->own.alloc_zeroed(&c->K, (size_t)batch * kRow, c->stream)) return fin(rc);
  viekf_cam_intrinsics k;
  viekf_cam_intrinsics_default(&k);
  if (int rc = upload_sets(c, &k, 1)) return fin(rc);
  *out = c;
  return VIEKF_OK;
}

int viekf_cam_destroy(viekf_cam* c) {
  if (!c) return fail(VIEKF_ERR_INVALID, "camera model is null");
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  cam_delete(c);
  return VIEKF_OK;
}

int viekf_cam_dims(const viekf_cam* c, int32_t* batch, int32_t* sets) {
  if (!c) return fail(VIEKF_ERR_INVALID, "camera model is null");
  if (batch) *batch = c->B;
  if (sets) *sets = c->sets;
  return VIEKF_OK;
}

int viekf_cam_set_stream(viekf_cam* c, void* hip_stream) {
  if (!c) return fail(VIEKF_ERR_INVALID, "camera model is null");
  if (int rc = set_dev(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->own_stream) HIP_TRY(hipStreamDestroy(c->stream));
  c->own_stream = false;
  c->stream = static_cast<hipStream_t>(hip_stream);
  return VIEKF_OK;
}

int viekf_cam_sync(viekf_cam* c) {
  if (!c) return fail(VIEKF_ERR_INVALID, "camera model is null");
  if (int rc = set_dev(c)) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return VIEKF_OK;
}

int viekf_cam_set_intrinsics(viekf_cam* c, const viekf_cam_intrinsics* k, int32_t per_camera) {
  if (!c || !k) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = set_dev(c)) return rc;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, k) != hipSuccess) {
    (void)hipGetLastError();                      // (plain host memory the runtime has never seen)
  } else if (at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeArray) {
    return fail(VIEKF_ERR_INVALID, "intrinsics must be in host memory: r_valid is derived on the host");
  }
  return upload_sets(c, k, per_camera ? c->B : 1);
}

int viekf_cam_get_intrinsics(const viekf_cam* c, viekf_cam_intrinsics* k, double* r_valid) {
  if (!c) return fail(VIEKF_ERR_INVALID, "camera model is null");
  for (int s = 0; s < c->sets; s++) {
    if (k) k[s] = c->k[s];
    if (r_valid) r_valid[s] = c->r_valid[s];
  }
  return VIEKF_OK;
}

int viekf_cam_distort_points(viekf_cam* c, int32_t M, const double* z_ideal, double* z_raw, double* J, viekf_mem where) {
  if (!c || !z_ideal || !z_raw) return fail(VIEKF_ERR_INVALID, "null argument (z_ideal and z_raw are required)");
  if (M < 1 || M > VIEKF_CAM_MAX_M) return fail(VIEKF_ERR_INVALID, "M must be in [1, VIEKF_CAM_MAX_M]");
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && (misaligned(z_ideal, 8) || misaligned(z_raw, 8) || misaligned(J, 8)))
    return fail(VIEKF_ERR_INVALID, "device arrays of doubles must be 8-byte aligned");
  if (int rc = set_dev(c)) return rc;
  const size_t n = (size_t)c->B * M;
  const double* di = z_ideal;
  double *dr = z_raw, *dj = J;
  if (where == VIEKF_HOST) {
    double *si = nullptr, *so = nullptr;          // stage 0: z_ideal; stage 1: z_raw | J
    if (int rc = cam_stage(c, 0, 16 * n, &si)) return rc;
    if (int rc = cam_stage(c, 1, 48 * n, &so)) return rc;
    if (int rc = copy_user(si, z_ideal, 16 * n, where, Copy::FromUser, c->stream)) return rc;
    di = si; dr = so; dj = J ? so + 2 * n : nullptr;
  }
  k_cam_distort<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->K, c->sets > 1, c->B, M, di, dr, dj);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    int rc;
    if ((rc = copy_user(z_raw, dr, 16 * n, where, Copy::ToUser, c->stream)) || (rc = copy_user(J, dj, 32 * n, where, Copy::ToUser, c->stream)))
      return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return VIEKF_OK;
}

int viekf_cam_undistort_points(viekf_cam* c, int32_t M, const double* z_raw, const double* R, int32_t r_mode, double* z_ideal,
                               double* R_out, int32_t* status, viekf_mem where) {
  if (!c || !z_raw || !z_ideal) return fail(VIEKF_ERR_INVALID, "null argument (z_raw and z_ideal are required)");
  if (M < 1 || M > VIEKF_CAM_MAX_M) return fail(VIEKF_ERR_INVALID, "M must be in [1, VIEKF_CAM_MAX_M]");
  if (R_out && !R) return fail(VIEKF_ERR_INVALID, "R_out needs R");
  if (R_out && (r_mode < 0 || r_mode > 2)) return fail(VIEKF_ERR_INVALID, "r_mode must be 0, 1 or 2");
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && (misaligned(z_raw, 8) || misaligned(z_ideal, 8) || misaligned(R, 8) || misaligned(R_out, 8) || misaligned(status, 4)))
    return fail(VIEKF_ERR_INVALID, "device arrays of doubles must be 8-byte and status 4-byte aligned");
  if (int rc = set_dev(c)) return rc;
  const size_t n = (size_t)c->B * M;
  const size_t rn = !R_out ? 0 : (r_mode == 0 ? 4 : (r_mode == 1 ? 4 * (size_t)c->B : 4 * n));
  const double *dz = z_raw, *dR = R_out ? R : nullptr;
  double *di = z_ideal, *dRo = R_out;
  int* ds = status;
  if (where == VIEKF_HOST) {
    double *sin_ = nullptr, *sout = nullptr;      // stage 0: z_raw | R; stage 1: z_ideal | R_out | status
    if (int rc = cam_stage(c, 0, 16 * n + 8 * rn, &sin_)) return rc;
    if (int rc = cam_stage(c, 1, 52 * n, &sout)) return rc;
    if (int rc = copy_user(sin_, z_raw, 16 * n, where, Copy::FromUser, c->stream)) return rc;
    if (R_out)
      if (int rc = copy_user(sin_ + 2 * n, R, 8 * rn, where, Copy::FromUser, c->stream)) return rc;
    dz = sin_; dR = R_out ? sin_ + 2 * n : nullptr;
    di = sout; dRo = R_out ? sout + 2 * n : nullptr; ds = status ? reinterpret_cast<int*>(sout + 6 * n) : nullptr;
  }
  k_cam_undistort<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->K, c->sets > 1, c->B, M, dz, dR, r_mode, di, dRo, ds);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    int rc;
    if ((rc = copy_user(z_ideal, di, 16 * n, where, Copy::ToUser, c->stream)) || (rc = copy_user(R_out, dRo, 32 * n, where, Copy::ToUser, c->stream)) ||
        (rc = copy_user(status, ds, 4 * n, where, Copy::ToUser, c->stream)))
      return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return VIEKF_OK;
}

int viekf_cam_valid_mask(viekf_cam* c, int32_t width, int32_t height, uint8_t* mask, viekf_mem where) {
  if (!c || !mask) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = check_image(width, height)) return rc;
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && misaligned(mask, 4)) return fail(VIEKF_ERR_INVALID, "mask must be 4-byte aligned");
  if (int rc = set_dev(c)) return rc;
  const size_t npx = (size_t)c->sets * width * height;
  uint8_t* dm = mask;
  if (where == VIEKF_HOST)
    if (int rc = cam_stage(c, 0, npx, &dm)) return rc;
  const int tx = (width + kTileW - 1) / kTileW, ty = (height + kTileH - 1) / kTileH;
  k_cam_mask<<<dim3((unsigned)(tx * ty), (unsigned)c->sets), 256, 0, c->stream>>>(c->K, width, height, tx, dm);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    if (int rc = copy_user(mask, dm, npx, where, Copy::ToUser, c->stream)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return VIEKF_OK;
}

int viekf_cam_warp(viekf_cam* c, int32_t direction, int32_t width, int32_t height, const uint8_t* src, uint8_t* dst, const float* src_depth,
                   float* dst_depth, int32_t fill, viekf_mem where) {
  if (!c || !src || !dst) return fail(VIEKF_ERR_INVALID, "null argument (src and dst are required)");
  if (direction != VIEKF_CAM_RECTIFY && direction != VIEKF_CAM_DISTORT) return fail(VIEKF_ERR_INVALID, "direction must be VIEKF_CAM_RECTIFY or VIEKF_CAM_DISTORT");
  if ((src_depth == nullptr) != (dst_depth == nullptr)) return fail(VIEKF_ERR_INVALID, "src_depth and dst_depth are given together or not at all");
  if (fill < 0 || fill > 255) return fail(VIEKF_ERR_INVALID, "fill must be in [0, 255]");
  if (int rc = check_image(width, height)) return rc;
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && (misaligned(dst, 4) || misaligned(dst_depth, 16) || misaligned(src_depth, 4)))
    return fail(VIEKF_ERR_INVALID, "dst must be 4-byte, dst_depth 16-byte and src_depth 4-byte aligned");
  if (int rc = set_dev(c)) return rc;
  const size_t npx = (size_t)c->B * width * height;
  const uint8_t* ds = src;
  uint8_t* dd = dst;
  const float* dsd = src_depth;
  float* ddd = dst_depth;
  if (where == VIEKF_HOST) {
    uint8_t* s0 = nullptr;
    float* s2 = nullptr;
    if (int rc = cam_stage(c, 0, npx, &s0)) return rc;
    if (int rc = cam_stage(c, 1, npx, &dd)) return rc;
    if (int rc = copy_user(s0, src, npx, where, Copy::FromUser, c->stream)) return rc;
    ds = s0;
    if (src_depth) {
      if (int rc = cam_stage(c, 2, 4 * npx, &s2)) return rc;
      if (int rc = cam_stage(c, 3, 4 * npx, &ddd)) return rc;
      if (int rc = copy_user(s2, src_depth, 4 * npx, where, Copy::FromUser, c->stream)) return rc;
      dsd = s2;
    }
  }
  const int tx = (width + kTileW - 1) / kTileW, ty = (height + kTileH - 1) / kTileH;
  const dim3 grid((unsigned)(tx * ty), (unsigned)c->B);
  if (direction == VIEKF_CAM_RECTIFY)
    k_cam_warp<VIEKF_CAM_RECTIFY><<<grid, 256, 0, c->stream>>>(c->K, c->sets > 1, width, height, tx, (unsigned)fill, ds, dd, dsd, ddd);
  else
    k_cam_warp<VIEKF_CAM_DISTORT><<<grid, 256, 0, c->stream>>>(c->K, c->sets > 1, width, height, tx, (unsigned)fill, ds, dd, dsd, ddd);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    int rc;
    if ((rc = copy_user(dst, dd, npx, where, Copy::ToUser, c->stream)) || (rc = copy_user(dst_depth, ddd, 4 * npx, where, Copy::ToUser, c->stream))) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return VIEKF_OK;
}

}  // extern "C"
