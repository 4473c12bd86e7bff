// viekf_klt.hip -- the batched KLT feature tracker behind include/viekf_klt.h: the reference's
// KLT_Tracker::load_image (src/klt_tracker.cpp:54-170) for B cameras, device-resident between frames.
//
// One frame is a fixed sequence of launches on the tracker's stream, with no host round trip:
//   k_grey       grey (BGR2GRAY), 180-degree flip and pyramid level 0 of the current pyramid
//   k_pyrdown    one launch per level (5x5 [1 4 6 4 1] kernel, REFLECT_101)
//   k_lk         pyramidal LK, one wavefront per (camera, point), Scharr derivatives from an LDS patch
//   k_prune      one wavefront per camera: status / border / mask / neighbour prune, how many corners to replenish
//   k_corner<1>  Sobel, 7x7 structure sums and the min-eigenvalue score per 16x16 LDS tile; masked maximum per camera
//   k_corner<2>  the score again, threshold, 3x3 maximum and mask; candidates appended as (score bits, raster index)
//   k_select     one workgroup per camera: sort (LDS, or global memory when it does not fit), greedy radius walk,
//                ids, outputs, and the swap of the two pyramids
// Compiled with -ffp-contract=off: the corner score is specified without FMAs, and the LK arithmetic then rounds
// operation by operation like the numpy restatement (tests/klt_ref.py).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/viekf_klt.h"
#include "viekf_hostkit.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kWin = 21, kHalf = 10, kMaxLevel = 3, kIters = 30;
constexpr int kTile = 16;               // corner tile: 16x16 scores, 18x18 with the 3x3 maximum's halo, 24x24 gradients
constexpr int kLdsKeys = 8192;          // candidates sorted in LDS (8 + 4 bytes each: 96 KiB); more go through global memory
constexpr int kSelThreads = 1024;

struct KltDev {
  int B, W, H, MF, R, invert, nlev;
  int lw[kMaxLevel + 1], lh[kMaxLevel + 1];
  long long loff[kMaxLevel + 1];
  long long pyr_sz;                     // bytes of one camera's pyramid
  long long ccap;                       // candidate capacity per camera: (W-2)(H-2), every interior pixel
  int mask_per_cam;
  uint8_t* pyr;                         // [2][B][pyr_sz]
  int* par;                             // [B] which half holds the PREVIOUS pyramid
  const uint8_t* mask;                  // [1 or B][H][W], 0 / 255
  const uint8_t* active;                // [B]
  float* pts;                           // [B][MF][2] tracked points (unclamped)
  int* ids;                             // [B][MF]
  int* cnt;                             // [B]
  int* next_id;                         // [B]
  int* init;                            // [B]
  float* nxt;                           // [B][MF][2] LK result
  uint8_t* status;                      // [B][MF]
  int* need;                            // [B] corners to detect this frame
  unsigned long long* lmax;             // [B] bits of the masked maximum score
  unsigned long long* ckey;             // [B][ccap]
  unsigned* cidx;                       // [B][ccap]
  int* ccnt;                            // [B]
  double* feat;                         // [B][MF][2] outputs
  int* oids;                            // [B][MF]
  int* ocnt;                            // [B]
};

__host__ __device__ inline int reflect101(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  int p = 2 * n - 2;
  i %= p;
  if (i < 0) i += p;
  return i >= n ? p - i : i;
}

__device__ inline const uint8_t* level_ptr(const KltDev& k, int half, int b, int l) {
  return k.pyr + ((long long)half * k.B + b) * k.pyr_sz + k.loff[l];
}

__device__ inline float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- grey + flip + level 0 ---------------------------------------------------------------------------------------------
// 4 pixels of one row per thread (W is not required to be a multiple of 4)
__global__ __launch_bounds__(256) void k_grey(KltDev k, const uint8_t* __restrict__ img, int ch) {
  const int b = blockIdx.y;
  if (!k.active[b]) return;
  const int qw = (k.W + 3) >> 2;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= qw * k.H) return;
  const int y = q / qw, x0 = (q - y * qw) * 4;
  const int sy = k.invert ? k.H - 1 - y : y;
  const uint8_t* src = img + ((long long)b * k.H + sy) * k.W * ch;
  uint8_t* dst = const_cast<uint8_t*>(level_ptr(k, 1 - k.par[b], b, 0)) + (long long)y * k.W;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int x = x0 + j;
    if (x >= k.W) break;
    const int sx = k.invert ? k.W - 1 - x : x;
    int g;
    if (ch == 1) {
      g = src[sx];
    } else {
      const uint8_t* p = src + sx * 3;
      g = (1868 * p[0] + 9617 * p[1] + 4899 * p[2] + 8192) >> 14;
    }
    dst[x] = (uint8_t)g;
  }
}

// ---- pyrDown: level l from level l-1 of the current pyramid -------------------------------------------------------------
__global__ __launch_bounds__(256) void k_pyrdown(KltDev k, int l) {
  const int b = blockIdx.y;
  if (!k.active[b]) return;
  const int w = k.lw[l], h = k.lh[l], sw = k.lw[l - 1], sh = k.lh[l - 1];
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= w * h) return;
  const int y = p / w, x = p - y * w;
  const int half = 1 - k.par[b];
  const uint8_t* src = level_ptr(k, half, b, l - 1);
  const int kw[5] = {1, 4, 6, 4, 1};
  int xs[5];
#pragma unroll
  for (int i = 0; i < 5; i++) xs[i] = reflect101(2 * x - 2 + i, sw);
  int s = 0;
#pragma unroll
  for (int j = 0; j < 5; j++) {
    const uint8_t* row = src + (long long)reflect101(2 * y - 2 + j, sh) * sw;
    int t = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) t += kw[i] * row[xs[i]];
    s += kw[j] * t;
  }
  const_cast<uint8_t*>(level_ptr(k, half, b, l))[p] = (uint8_t)((s + 128) >> 8);
}

// ---- pyramidal LK: one wavefront per (camera, point) -------------------------------------------------------------------
__device__ inline bool lk_out(int ix, int iy, int w, int h) { return ix < -kWin || ix >= w || iy < -kWin || iy >= h; }

__global__ __launch_bounds__(64) void k_lk(KltDev k) {
  const int b = blockIdx.y, i = blockIdx.x, lane = threadIdx.x;
  if (!k.active[b] || !k.init[b] || i >= k.cnt[b]) return;
  __shared__ float patch[24 * 24];      // prev level at floor(prev) - 1 + [0, 24)^2, REFLECT_101 reads
  __shared__ float sdx[22 * 22], sdy[22 * 22];   // Scharr at floor(prev) + [0, 22)^2, 0 outside the level
  const int pv = k.par[b], cu = 1 - pv;
  const float px0 = k.pts[((long long)b * k.MF + i) * 2], py0 = k.pts[((long long)b * k.MF + i) * 2 + 1];
  float nox = 0.f, noy = 0.f;           // nextPts[i] (level coordinates)
  bool status = true;
  const float FLT_SCALE = 1.0f / (1 << 20);
  for (int l = k.nlev - 1; l >= 0; l--) {
    const int w = k.lw[l], h = k.lh[l];
    const uint8_t* I = level_ptr(k, pv, b, l);
    const uint8_t* J = level_ptr(k, cu, b, l);
    const float sc = 1.0f / (float)(1 << l);
    float prx = px0 * sc, pry = py0 * sc;
    float nx, ny;
    if (l == k.nlev - 1) { nx = prx; ny = pry; } else { nx = nox * 2.f; ny = noy * 2.f; }
    nox = nx; noy = ny;
    prx -= (float)kHalf; pry -= (float)kHalf;
    const int ipx = (int)floorf(prx), ipy = (int)floorf(pry);
    if (lk_out(ipx, ipy, w, h)) { if (l == 0) status = false; continue; }
    const float a = prx - (float)ipx, bb = pry - (float)ipy;
    const float w00 = (1.f - a) * (1.f - bb), w01 = a * (1.f - bb), w10 = (1.f - a) * bb, w11 = a * bb;
    __syncthreads();
    for (int t = lane; t < 24 * 24; t += 64) {
      const int r = t / 24, c = t - r * 24;
      patch[t] = (float)I[(long long)reflect101(ipy - 1 + r, h) * w + reflect101(ipx - 1 + c, w)];
    }
    __syncthreads();
    for (int t = lane; t < 22 * 22; t += 64) {
      const int r = t / 22, c = t - r * 22;
      const int gx = ipx + c, gy = ipy + r;
      float dx = 0.f, dy = 0.f;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
        const float* p0 = patch + r * 24 + c;          // (gx-1, gy-1)
        const float* p1 = p0 + 24;
        const float* p2 = p1 + 24;
        dx = 3.f * (p0[2] - p0[0]) + 10.f * (p1[2] - p1[0]) + 3.f * (p2[2] - p2[0]);
        dy = 3.f * (p2[0] - p0[0]) + 10.f * (p2[1] - p0[1]) + 3.f * (p2[2] - p0[2]);
      }
      sdx[t] = dx;
      sdy[t] = dy;
    }
    __syncthreads();
    float iv[7], gx7[7], gy7[7];
    float s11 = 0.f, s12 = 0.f, s22 = 0.f;
#pragma unroll
    for (int s = 0; s < 7; s++) {
      const int t = lane + 64 * s;
      iv[s] = gx7[s] = gy7[s] = 0.f;
      if (t < kWin * kWin) {
        const int wy = t / kWin, wx = t - wy * kWin;
        const float* p = patch + (wy + 1) * 24 + wx + 1;
        iv[s] = (((w00 * p[0] + w01 * p[1]) + w10 * p[24]) + w11 * p[25]) * 32.f;
        const float* q = sdx + wy * 22 + wx;
        gx7[s] = ((w00 * q[0] + w01 * q[1]) + w10 * q[22]) + w11 * q[23];
        q = sdy + wy * 22 + wx;
        gy7[s] = ((w00 * q[0] + w01 * q[1]) + w10 * q[22]) + w11 * q[23];
        s11 += gx7[s] * gx7[s];
        s12 += gx7[s] * gy7[s];
        s22 += gy7[s] * gy7[s];
      }
    }
    const float A11 = wave_sum(s11) * FLT_SCALE, A12 = wave_sum(s12) * FLT_SCALE, A22 = wave_sum(s22) * FLT_SCALE;
    const float D = A11 * A22 - A12 * A12;
    const float mev = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * kWin * kWin);
    if (mev < 1e-4f || D < FLT_EPSILON) { if (l == 0) status = false; continue; }
    const float Dinv = 1.f / D;
    float cx = nx - (float)kHalf, cy = ny - (float)kHalf, pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < kIters; j++) {
      const int inx = (int)floorf(cx), iny = (int)floorf(cy);
      if (lk_out(inx, iny, w, h)) { if (l == 0) status = false; break; }
      const float ja = cx - (float)inx, jb = cy - (float)iny;
      const float v00 = (1.f - ja) * (1.f - jb), v01 = ja * (1.f - jb), v10 = (1.f - ja) * jb, v11 = ja * jb;
      float b1 = 0.f, b2 = 0.f;
#pragma unroll
      for (int s = 0; s < 7; s++) {
        const int t = lane + 64 * s;
        if (t < kWin * kWin) {
          const int wy = t / kWin, wx = t - wy * kWin;
          const int x0 = reflect101(inx + wx, w), x1 = reflect101(inx + wx + 1, w);
          const uint8_t* r0 = J + (long long)reflect101(iny + wy, h) * w;
          const uint8_t* r1 = J + (long long)reflect101(iny + wy + 1, h) * w;
          const float jv = (((v00 * (float)r0[x0] + v01 * (float)r0[x1]) + v10 * (float)r1[x0]) + v11 * (float)r1[x1]) * 32.f;
          const float diff = jv - iv[s];
          b1 += diff * gx7[s];
          b2 += diff * gy7[s];
        }
      }
      b1 = wave_sum(b1) * FLT_SCALE;
      b2 = wave_sum(b2) * FLT_SCALE;
      const float dx = (A12 * b2 - A22 * b1) * Dinv, dy = (A12 * b1 - A11 * b2) * Dinv;
      cx += dx;
      cy += dy;
      nox = cx + (float)kHalf;
      noy = cy + (float)kHalf;
      if ((double)dx * (double)dx + (double)dy * (double)dy <= 1e-4) break;
      if (j > 0 && fabsf(dx + pdx) < 0.01f && fabsf(dy + pdy) < 0.01f) {
        nox -= dx * 0.5f;
        noy -= dy * 0.5f;
        break;
      }
      pdx = dx;
      pdy = dy;
    }
  }
  if (lane == 0) {
    k.nxt[((long long)b * k.MF + i) * 2] = nox;
    k.nxt[((long long)b * k.MF + i) * 2 + 1] = noy;
    k.status[(long long)b * k.MF + i] = status ? 1 : 0;
  }
}

// ---- prune (klt_tracker.cpp:86-115, the intended neighbour test) and how many corners to replenish ------------------------
__global__ __launch_bounds__(64) void k_prune(KltDev k) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (!k.active[b]) return;
  if (lane == 0) { k.lmax[b] = 0ull; k.ccnt[b] = 0; }
  if (!k.init[b]) {
    if (lane == 0) { k.cnt[b] = 0; k.need[b] = k.MF; }
    return;
  }
  __shared__ float kx[VIEKF_KLT_MAX_FEATURES], ky[VIEKF_KLT_MAX_FEATURES];
  __shared__ int kidx[VIEKF_KLT_MAX_FEATURES];
  const int n = k.cnt[b];
  const float* nxt = k.nxt + (long long)b * k.MF * 2;
  const uint8_t* mask = k.mask + (k.mask_per_cam ? (long long)b * k.W * k.H : 0ll);
  const double r = (double)k.R;
  int nk = 0;                           // kept so far, in visiting order (descending index)
  for (int i = n - 1; i >= 0; i--) {
    const double x = nxt[2 * i], y = nxt[2 * i + 1];
    // (written as "not inside" so that a non-finite position is dropped before it indexes the mask)
    bool drop = !k.status[(long long)b * k.MF + i] || !(x > 1.0 && y > 1.0 && x < k.W - 1.0 && y < k.H - 1.0);
    if (!drop) drop = mask[(long long)(int)round(y) * k.W + (int)round(x)] != 255;
    if (!drop) {
      bool close = false;
      for (int j = lane; j < nk; j += 64) {
        const double dx = (double)kx[j] - x, dy = (double)ky[j] - y;
        close |= sqrt(dx * dx + dy * dy) < r;
      }
      drop = __any(close);
    }
    if (!drop) {
      if (lane == 0) { kx[nk] = (float)x; ky[nk] = (float)y; kidx[nk] = i; }
      nk++;
    }
    __syncthreads();
  }
  // compact in the original order: the j-th kept point (ascending) is kidx[nk-1-j]
  int myid[VIEKF_KLT_MAX_FEATURES / 64];
#pragma unroll
  for (int s = 0; s < VIEKF_KLT_MAX_FEATURES / 64; s++) {
    const int j = lane + 64 * s;
    myid[s] = j < nk ? k.ids[(long long)b * k.MF + kidx[nk - 1 - j]] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < VIEKF_KLT_MAX_FEATURES / 64; s++) {
    const int j = lane + 64 * s;
    if (j < nk) {
      const int src = kidx[nk - 1 - j];
      k.ids[(long long)b * k.MF + j] = myid[s];
      k.pts[((long long)b * k.MF + j) * 2] = nxt[2 * src];
      k.pts[((long long)b * k.MF + j) * 2 + 1] = nxt[2 * src + 1];
    }
  }
  if (lane == 0) {
    k.cnt[b] = nk;
    k.need[b] = nk < k.MF ? k.MF - nk : 0;
  }
}

// ---- corner score per tile (goodFeaturesToTrack's cornerMinEigenVal, block 7, Sobel 3) ----------------------------------
template <int PASS>
__global__ __launch_bounds__(256) void k_corner(KltDev k) {
  const int b = blockIdx.y, tid = threadIdx.x;
  if (!k.active[b] || k.need[b] == 0) return;
  const int tilesX = (k.W + kTile - 1) / kTile;
  const int tx0 = (blockIdx.x % tilesX) * kTile, ty0 = (blockIdx.x / tilesX) * kTile;
  const int W = k.W, H = k.H;
  __shared__ int sa[24 * 24], sb[24 * 24], sc[24 * 24];
  __shared__ int ha[24 * 18], hb[24 * 18], hc[24 * 18];
  __shared__ double lam[18 * 18];
  __shared__ int dxs[VIEKF_KLT_MAX_FEATURES], dys[VIEKF_KLT_MAX_FEATURES];
  __shared__ int ndisc;
  __shared__ unsigned long long wmax[4];
  const uint8_t* img = level_ptr(k, 1 - k.par[b], b, 0);
  const uint8_t* mask = k.mask + (k.mask_per_cam ? (long long)b * W * H : 0ll);
  // the kept points whose replenish disc (dx^2 + dy^2 <= r^2 around cvRound(p)) can touch this tile
  if (tid == 0) ndisc = 0;
  __syncthreads();
  const int nkept = k.init[b] ? k.cnt[b] : 0, R = k.R;
  for (int j = tid; j < nkept; j += 256) {
    const int cx = (int)rintf(k.pts[((long long)b * k.MF + j) * 2]), cy = (int)rintf(k.pts[((long long)b * k.MF + j) * 2 + 1]);
    if (cx + R >= tx0 && cx - R < tx0 + kTile && cy + R >= ty0 && cy - R < ty0 + kTile) {
      const int s = atomicAdd(&ndisc, 1);
      dxs[s] = cx;
      dys[s] = cy;
    }
  }
  // Sobel at tile - 4 + [0, 24)^2; the gradient planes are extended with REFLECT_101 as well
  for (int t = tid; t < 24 * 24; t += 256) {
    const int r = t / 24, c = t - r * 24;
    const int x = reflect101(tx0 - 4 + c, W), y = reflect101(ty0 - 4 + r, H);
    const int xm = reflect101(x - 1, W), xp = reflect101(x + 1, W);
    const uint8_t* rm = img + (long long)reflect101(y - 1, H) * W;
    const uint8_t* r0 = img + (long long)y * W;
    const uint8_t* rp = img + (long long)reflect101(y + 1, H) * W;
    const int dx = (rm[xp] - rm[xm]) + 2 * (r0[xp] - r0[xm]) + (rp[xp] - rp[xm]);
    const int dy = (rp[xm] - rm[xm]) + 2 * (rp[x] - rm[x]) + (rp[xp] - rm[xp]);
    sa[t] = dx * dx;
    sb[t] = dx * dy;
    sc[t] = dy * dy;
  }
  __syncthreads();
  for (int t = tid; t < 24 * 18; t += 256) {
    const int r = t / 18, c = t - r * 18;
    int A = 0, Bv = 0, Cv = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) { A += sa[r * 24 + c + i]; Bv += sb[r * 24 + c + i]; Cv += sc[r * 24 + c + i]; }
    ha[t] = A; hb[t] = Bv; hc[t] = Cv;
  }
  __syncthreads();
  for (int t = tid; t < 18 * 18; t += 256) {
    const int r = t / 18, c = t - r * 18;
    int A = 0, Bv = 0, Cv = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) { A += ha[(r + i) * 18 + c]; Bv += hb[(r + i) * 18 + c]; Cv += hc[(r + i) * 18 + c]; }
    const long long am = (long long)A - Cv;
    const long long D = am * am + 4ll * Bv * Bv;
    const double v = 0.5 * ((double)(A + Cv) - sqrt((double)D));
    lam[t] = v > 0.0 ? v : 0.0;
  }
  __syncthreads();
  // this thread's pixel
  const int ly = tid / kTile, lx = tid - ly * kTile;
  const int x = tx0 + lx, y = ty0 + ly;
  const bool in = x < W && y < H;
  bool usable = false;
  if (in) {
    usable = mask[(long long)y * W + x] != 0;
    for (int j = 0; j < ndisc && usable; j++) {
      const int ex = x - dxs[j], ey = y - dys[j];
      usable = ex * ex + ey * ey > R * R;
    }
  }
  const double v = lam[(ly + 1) * 18 + lx + 1];
  if (PASS == 1) {
    unsigned long long m = usable ? (unsigned long long)__double_as_longlong(v) : 0ull;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const unsigned long long u = __shfl_xor(m, o, 64);
      m = u > m ? u : m;
    }
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
      unsigned long long mm = wmax[0];
      for (int i = 1; i < 4; i++) mm = wmax[i] > mm ? wmax[i] : mm;
      if (mm) atomicMax(&k.lmax[b], mm);
    }
  } else {
    const double thr = 0.3 * __longlong_as_double((long long)k.lmax[b]);
    auto lp = [&](int r, int c) { const double u = lam[r * 18 + c]; return u > thr ? u : 0.0; };
    const double me = lp(ly + 1, lx + 1);
    bool cand = in && usable && x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && me != 0.0;
    if (cand) {
#pragma unroll
      for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) cand &= lp(ly + dy, lx + dx) <= me;
    }
    const unsigned long long bal = __ballot(cand);
    if (bal) {
      const int lane = tid & 63;
      int base = 0;
      if (lane == __ffsll((long long)bal) - 1) base = atomicAdd(&k.ccnt[b], __popcll(bal));
      base = __shfl(base, __ffsll((long long)bal) - 1, 64);
      if (cand) {
        const long long pos = base + __popcll(bal & ((1ull << lane) - 1ull));
        if (pos < k.ccap) {
          k.ckey[(long long)b * k.ccap + pos] = (unsigned long long)__double_as_longlong(me);
          k.cidx[(long long)b * k.ccap + pos] = (unsigned)(y * W + x);
        }
      }
    }
  }
}

// ---- selection: sort, greedy radius walk, ids, outputs --------------------------------------------------------------------
// "a goes before b": score descending, then raster index ascending
__device__ inline bool before(unsigned long long ka, unsigned ia, unsigned long long kb, unsigned ib) {
  return ka > kb || (ka == kb && ia < ib);
}

// Same-direction bitonic network over n keys (virtual padding to a power of two: the padding is "last" and never moves)
__device__ void sort_keys(unsigned long long* key, unsigned* idx, int n) {
  int P = 1;
  while (P < n) P <<= 1;
  for (int kk = 2; kk <= P; kk <<= 1) {
    for (int t = threadIdx.x; t < P / 2; t += blockDim.x) {
      const int hk = kk >> 1, blk = t / hk, off = t - blk * hk;
      const int lo = blk * kk + off, hi = blk * kk + kk - 1 - off;
      if (hi < n && before(key[hi], idx[hi], key[lo], idx[lo])) {
        const unsigned long long a = key[lo]; key[lo] = key[hi]; key[hi] = a;
        const unsigned c = idx[lo]; idx[lo] = idx[hi]; idx[hi] = c;
      }
    }
    __syncthreads();
    for (int j = kk >> 2; j >= 1; j >>= 1) {
      for (int t = threadIdx.x; t < P / 2; t += blockDim.x) {
        const int blk = t / j, off = t - blk * j;
        const int lo = blk * 2 * j + off, hi = lo + j;
        if (hi < n && before(key[hi], idx[hi], key[lo], idx[lo])) {
          const unsigned long long a = key[lo]; key[lo] = key[hi]; key[hi] = a;
          const unsigned c = idx[lo]; idx[lo] = idx[hi]; idx[hi] = c;
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(kSelThreads) void k_select(KltDev k) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (!k.active[b]) return;
  extern __shared__ __align__(16) unsigned char dyn[];
  __shared__ int ax[VIEKF_KLT_MAX_FEATURES], ay[VIEKF_KLT_MAX_FEATURES];
  __shared__ int nacc_s;
  const int need = k.need[b];
  const int cnt0 = k.cnt[b];
  if (tid == 0) nacc_s = 0;
  if (need > 0) {
    const int n = (int)min((long long)k.ccnt[b], k.ccap);
    unsigned long long* key = k.ckey + (long long)b * k.ccap;
    unsigned* idx = k.cidx + (long long)b * k.ccap;
    if (n <= kLdsKeys) {
      unsigned long long* lk = reinterpret_cast<unsigned long long*>(dyn);
      unsigned* li = reinterpret_cast<unsigned*>(dyn + kLdsKeys * sizeof(unsigned long long));
      for (int t = tid; t < n; t += blockDim.x) { lk[t] = key[t]; li[t] = idx[t]; }
      __syncthreads();
      key = lk;
      idx = li;
    }
    sort_keys(key, idx, n);
    if (tid < 64) {                     // one wavefront walks the sorted candidates, 64 at a time
      const int r2 = k.R * k.R;
      int nacc = 0;
      for (int c0 = 0; c0 < n && nacc < need; c0 += 64) {
        const int c = c0 + tid;
        int x = 0, y = 0;
        bool ok = c < n;
        if (ok) {
          const unsigned p = idx[c];
          y = (int)(p / (unsigned)k.W);
          x = (int)(p - (unsigned)y * (unsigned)k.W);
          for (int j = 0; j < nacc && ok; j++) {
            const int ex = x - ax[j], ey = y - ay[j];
            ok = ex * ex + ey * ey >= r2;
          }
        }
        unsigned long long m = __ballot(ok);
        while (m && nacc < need) {
          const int L = __ffsll((long long)m) - 1;
          const int lx = __shfl(x, L, 64), lyy = __shfl(y, L, 64);
          if (tid == 0) { ax[nacc] = lx; ay[nacc] = lyy; }
          nacc++;
          if (tid <= L) ok = false;
          else if (ok) { const int ex = x - lx, ey = y - lyy; ok = ex * ex + ey * ey >= r2; }
          m = __ballot(ok);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (ax / ay written by lane 0 are read by every lane next chunk)
      }
      if (tid == 0) nacc_s = nacc;
    }
  }
  __syncthreads();
  const int nacc = nacc_s;
  const int nid = k.next_id[b];
  for (int j = tid; j < nacc; j += blockDim.x) {
    k.pts[((long long)b * k.MF + cnt0 + j) * 2] = (float)ax[j];
    k.pts[((long long)b * k.MF + cnt0 + j) * 2 + 1] = (float)ay[j];
    k.ids[(long long)b * k.MF + cnt0 + j] = nid + j;
  }
  __syncthreads();
  const int total = cnt0 + nacc;
  for (int j = tid; j < k.MF; j += blockDim.x) {
    double fx = __longlong_as_double(0x7ff8000000000000ll), fy = fx;
    int id = -1;
    if (j < total) {
      fx = k.pts[((long long)b * k.MF + j) * 2];
      fy = k.pts[((long long)b * k.MF + j) * 2 + 1];
      fx = fx > k.W ? (double)k.W : fx < 0.0 ? 0.0 : fx;
      fy = fy > k.H ? (double)k.H : fy < 0.0 ? 0.0 : fy;
      id = k.ids[(long long)b * k.MF + j];
    }
    k.feat[((long long)b * k.MF + j) * 2] = fx;
    k.feat[((long long)b * k.MF + j) * 2 + 1] = fy;
    k.oids[(long long)b * k.MF + j] = id;
  }
  if (tid == 0) {
    k.cnt[b] = total;
    k.ocnt[b] = total;
    k.next_id[b] = nid + nacc;
    k.init[b] = 1;
    k.par[b] = 1 - k.par[b];            // this frame's pyramid is the next frame's prev
  }
}

// ---- small kernels ---------------------------------------------------------------------------------------------------
__global__ void k_mask(uint8_t* m, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) m[i] = m[i] > 1 ? 255 : 0;
}

__global__ void k_fill_active(uint8_t* a, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) a[i] = 1;
}

// drop_feature for every listed id, the point and its id together (one thread per camera)
__global__ void k_drop(KltDev k, const int* __restrict__ drop, int dcnt, uint8_t* found) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= k.B) return;
  int n = k.cnt[b];
  int* ids = k.ids + (long long)b * k.MF;
  float* pts = k.pts + (long long)b * k.MF * 2;
  for (int q = 0; q < dcnt; q++) {
    const int id = drop[(long long)b * dcnt + q];
    int at = -1;
    if (id >= 0)
      for (int i = 0; i < n; i++)
        if (ids[i] == id) { at = i; break; }
    if (at >= 0) {
      for (int i = at; i + 1 < n; i++) { ids[i] = ids[i + 1]; pts[2 * i] = pts[2 * i + 2]; pts[2 * i + 1] = pts[2 * i + 3]; }
      n--;
    }
    found[(long long)b * dcnt + q] = at >= 0 ? 1 : 0;
  }
  k.cnt[b] = n;
}

__global__ void k_depth(KltDev k, const float* __restrict__ dimg, double min_depth, double* out) {
  const int b = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
  if (i >= k.MF) return;
  double z = __longlong_as_double(0x7ff8000000000000ll);
  if (i < k.ocnt[b]) {
    int x = (int)round(k.feat[((long long)b * k.MF + i) * 2]), y = (int)round(k.feat[((long long)b * k.MF + i) * 2 + 1]);
    x = min(max(x, 0), k.W - 1);
    y = min(max(y, 0), k.H - 1);
    if (k.invert) { x = k.W - 1 - x; y = k.H - 1 - y; }
    const float d = (float)((double)dimg[((long long)b * k.H + y) * k.W + x] * 1e-3);
    z = (d > 1e3 || d < min_depth) ? z : (double)d;
  }
  out[(long long)b * k.MF + i] = z;
}

__global__ void k_get_level(KltDev k, int l, uint8_t* out) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, n = k.lw[l] * k.lh[l];
  if (p < n) out[(long long)b * n + p] = level_ptr(k, k.par[b], b, l)[p];
}

}  // namespace

struct viekf_klt {
  KltDev d{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevOwner own;                         // every device buffer of d and below
  uint8_t* img = nullptr;               // staging of host frames [B][H][W][3]
  float* dimg = nullptr;                // staging of host depth images [B][H][W]
  double* depth = nullptr;              // [B][MF]
};

namespace {

// the end of a tracker (the caller has set the device and waited for its stream)
void klt_delete(viekf_klt* k) {
  k->own.release_all();
  if (k->own_stream && k->stream) (void)hipStreamDestroy(k->stream);
  delete k;
}

// the padded outputs of a camera that has not run a frame: NaN, -1, 0
int klt_clear_outputs(viekf_klt* k) {
  const KltDev& d = k->d;
  HIP_TRY(hipMemsetAsync(d.feat, 0xff, sizeof(double) * d.B * d.MF * 2, k->stream));   // (all-ones bits: a NaN)
  HIP_TRY(hipMemsetAsync(d.oids, 0xff, sizeof(int) * d.B * d.MF, k->stream));
  HIP_TRY(hipMemsetAsync(d.ocnt, 0, sizeof(int) * d.B, k->stream));
  return VIEKF_OK;
}

int copy_out(viekf_klt* k, void* dst, const void* src, size_t bytes, viekf_mem where) {
  return copy_user(dst, src, bytes, where, Copy::ToUser, k->stream);
}

int set_dev(const viekf_klt* k) {
  HIP_TRY(hipSetDevice(k->device));
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int viekf_klt_create(int32_t batch, int32_t width, int32_t height, int32_t max_features, int32_t radius, int32_t invert_image,
                     int32_t device, viekf_klt** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "out is null");
  *out = nullptr;
  if (batch <= 0 || batch > 65535) return fail(VIEKF_ERR_INVALID, "batch must be in [1, 65535]");
  if (width < 8 || height < 8 || width > 16384 || height > 16384) return fail(VIEKF_ERR_INVALID, "width and height must be in [8, 16384]");
  if (max_features < 1 || max_features > VIEKF_KLT_MAX_FEATURES) return fail(VIEKF_ERR_INVALID, "max_features must be in [1, 1024]");
  if (radius < 0 || radius > 1024) return fail(VIEKF_ERR_INVALID, "radius must be in [0, 1024]");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(VIEKF_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  }
  if (device < 0 || device >= ndev) return fail(VIEKF_ERR_NO_DEVICE, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  viekf_klt* k = new viekf_klt();
  k->device = device;
  KltDev& d = k->d;
  d.B = batch; d.W = width; d.H = height; d.MF = max_features; d.R = radius; d.invert = invert_image != 0;
  // levels while the next one is larger than the window in both dimensions (buildOpticalFlowPyramid), at most 3
  d.lw[0] = width; d.lh[0] = height; d.nlev = 1;
  while (d.nlev <= kMaxLevel) {
    const int w = (d.lw[d.nlev - 1] + 1) / 2, h = (d.lh[d.nlev - 1] + 1) / 2;
    if (w <= kWin || h <= kWin) break;
    d.lw[d.nlev] = w; d.lh[d.nlev] = h; d.nlev++;
  }
  long long off = 0;
  for (int l = 0; l < d.nlev; l++) { d.loff[l] = off; off += ((long long)d.lw[l] * d.lh[l] + 255) & ~255ll; }
  d.pyr_sz = off;
  d.ccap = (long long)(width - 2) * (height - 2);
  int rc = VIEKF_OK;
  auto fin = [&](int code) { klt_delete(k); return code; };
  if (hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking) != hipSuccess) return fin(fail(VIEKF_ERR_HIP, "hipStreamCreate failed"));
  k->own_stream = true;
  const long long B = batch, MF = max_features;
  auto zeroed = [&](auto** p, long long count) { return k->own.alloc_zeroed(p, (size_t)count, k->stream); };
  if ((rc = zeroed(&d.pyr, 2 * B * d.pyr_sz)) || (rc = zeroed(&d.par, B)) ||
      (rc = zeroed(&d.mask, B * width * height)) || (rc = zeroed(&d.active, B)) ||
      (rc = zeroed(&d.pts, 2 * B * MF)) || (rc = zeroed(&d.ids, B * MF)) || (rc = zeroed(&d.cnt, B)) ||
      (rc = zeroed(&d.next_id, B)) || (rc = zeroed(&d.init, B)) || (rc = zeroed(&d.nxt, 2 * B * MF)) ||
      (rc = zeroed(&d.status, B * MF)) || (rc = zeroed(&d.need, B)) || (rc = zeroed(&d.lmax, B)) ||
      (rc = zeroed(&d.ckey, B * d.ccap)) || (rc = zeroed(&d.cidx, B * d.ccap)) ||
      (rc = zeroed(&d.ccnt, B)) || (rc = zeroed(&d.feat, 2 * B * MF)) || (rc = zeroed(&d.oids, B * MF)) ||
      (rc = zeroed(&d.ocnt, B)) || (rc = zeroed(&k->depth, B * MF)))
    return fin(rc);
  if (hipMemsetAsync(const_cast<uint8_t*>(d.mask), 255, (size_t)B * width * height, k->stream) != hipSuccess ||
      klt_clear_outputs(k) != VIEKF_OK)
    return fin(fail(VIEKF_ERR_HIP, "initialising the tracker's buffers failed"));
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(k_select), hipFuncAttributeMaxDynamicSharedMemorySize,
                          kLdsKeys * 12) != hipSuccess ||
      hipStreamSynchronize(k->stream) != hipSuccess)
    return fin(fail(VIEKF_ERR_HIP, "tracker setup failed"));
  *out = k;
  return VIEKF_OK;
}

int viekf_klt_destroy(viekf_klt* k) {
  if (!k) return fail(VIEKF_ERR_INVALID, "tracker is null");
  (void)hipSetDevice(k->device);
  if (k->stream) (void)hipStreamSynchronize(k->stream);
  klt_delete(k);
  return VIEKF_OK;
}

int viekf_klt_dims(const viekf_klt* k, int32_t* batch, int32_t* width, int32_t* height, int32_t* max_features, int32_t* radius,
                   int32_t* levels) {
  if (!k) return fail(VIEKF_ERR_INVALID, "tracker is null");
  if (batch) *batch = k->d.B;
  if (width) *width = k->d.W;
  if (height) *height = k->d.H;
  if (max_features) *max_features = k->d.MF;
  if (radius) *radius = k->d.R;
  if (levels) *levels = k->d.nlev;
  return VIEKF_OK;
}

int viekf_klt_reset(viekf_klt* k) {
  if (!k) return fail(VIEKF_ERR_INVALID, "tracker is null");
  if (int rc = set_dev(k)) return rc;
  const KltDev& d = k->d;
  HIP_TRY(hipMemsetAsync(d.init, 0, 4 * d.B, k->stream));
  HIP_TRY(hipMemsetAsync(d.next_id, 0, 4 * d.B, k->stream));
  HIP_TRY(hipMemsetAsync(d.cnt, 0, 4 * d.B, k->stream));
  if (int rc = klt_clear_outputs(k)) return rc;
  HIP_TRY(hipStreamSynchronize(k->stream));
  return VIEKF_OK;
}

int viekf_klt_set_stream(viekf_klt* k, void* hip_stream) {
  if (!k) return fail(VIEKF_ERR_INVALID, "tracker is null");
  if (int rc = set_dev(k)) return rc;
  HIP_TRY(hipStreamSynchronize(k->stream));
  if (k->own_stream) HIP_TRY(hipStreamDestroy(k->stream));
  k->own_stream = false;
  k->stream = static_cast<hipStream_t>(hip_stream);
  return VIEKF_OK;
}

int viekf_klt_sync(viekf_klt* k) {
  if (!k) return fail(VIEKF_ERR_INVALID, "tracker is null");
  if (int rc = set_dev(k)) return rc;
  HIP_TRY(hipStreamSynchronize(k->stream));
  return VIEKF_OK;
}

int viekf_klt_set_mask(viekf_klt* k, const uint8_t* mask, int32_t per_camera, viekf_mem where) {
  if (!k || !mask) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(k)) return rc;
  KltDev& d = k->d;
  const long long n = (per_camera ? (long long)d.B : 1ll) * d.W * d.H;
  uint8_t* m = const_cast<uint8_t*>(d.mask);
  if (int rc = copy_user(m, mask, n, where, Copy::FromUser, k->stream)) return rc;
  k_mask<<<(unsigned)((n + 255) / 256), 256, 0, k->stream>>>(m, n);
  HIP_TRY(hipGetLastError());
  d.mask_per_cam = per_camera != 0;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(k->stream));
  return VIEKF_OK;
}

int viekf_klt_load_image(viekf_klt* k, const uint8_t* img, int32_t channels, const uint8_t* active, double* features,
                         int32_t* ids, int32_t* count, viekf_mem where) {
  if (!k || !img) return fail(VIEKF_ERR_INVALID, "null argument");
  if (channels != 1 && channels != 3) return fail(VIEKF_ERR_INVALID, "channels must be 1 (GRAY8) or 3 (BGR8)");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(k)) return rc;
  KltDev& d = k->d;
  const long long B = d.B, MF = d.MF;
  const uint8_t* src = img;
  if (where == VIEKF_HOST) {
    if (!k->img)
      if (int rc = k->own.alloc(&k->img, (size_t)B * d.W * d.H * 3)) return rc;
    HIP_TRY(hipMemcpyAsync(k->img, img, (size_t)B * d.W * d.H * channels, hipMemcpyHostToDevice, k->stream));
    src = k->img;
  }
  uint8_t* act = const_cast<uint8_t*>(d.active);
  if (active) {
    if (int rc = copy_user(act, active, B, where, Copy::FromUser, k->stream)) return rc;
  } else
    k_fill_active<<<(unsigned)((B + 255) / 256), 256, 0, k->stream>>>(act, (int)B);
  const unsigned qw = (d.W + 3) / 4;
  k_grey<<<dim3((qw * d.H + 255) / 256, B), 256, 0, k->stream>>>(d, src, channels);
  for (int l = 1; l < d.nlev; l++)
    k_pyrdown<<<dim3((d.lw[l] * d.lh[l] + 255) / 256, B), 256, 0, k->stream>>>(d, l);
  k_lk<<<dim3(MF, B), 64, 0, k->stream>>>(d);
  k_prune<<<B, 64, 0, k->stream>>>(d);
  const unsigned tiles = ((d.W + kTile - 1) / kTile) * ((d.H + kTile - 1) / kTile);
  k_corner<1><<<dim3(tiles, B), 256, 0, k->stream>>>(d);
  k_corner<2><<<dim3(tiles, B), 256, 0, k->stream>>>(d);
  k_select<<<B, kSelThreads, kLdsKeys * 12, k->stream>>>(d);
  HIP_TRY(hipGetLastError());
  if (int rc = copy_out(k, features, d.feat, sizeof(double) * B * MF * 2, where)) return rc;
  if (int rc = copy_out(k, ids, d.oids, sizeof(int) * B * MF, where)) return rc;
  if (int rc = copy_out(k, count, d.ocnt, sizeof(int) * B, where)) return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(k->stream));
  return VIEKF_OK;
}

int viekf_klt_drop_features(viekf_klt* k, const int32_t* ids, int32_t cnt, uint8_t* found) {
  if (!k || (!ids && cnt > 0)) return fail(VIEKF_ERR_INVALID, "null argument");
  if (cnt < 0) return fail(VIEKF_ERR_INVALID, "cnt must be >= 0");
  if (cnt == 0) return VIEKF_OK;
  if (int rc = set_dev(k)) return rc;
  const KltDev& d = k->d;
  const size_t n = (size_t)d.B * cnt;
  int* dids = nullptr;
  uint8_t* dfound = nullptr;
  HIP_TRY(hipMalloc(&dids, n * 4 + n));
  dfound = reinterpret_cast<uint8_t*>(dids + n);
  hipError_t e = hipMemcpyAsync(dids, ids, n * 4, hipMemcpyHostToDevice, k->stream);
  if (e == hipSuccess) {
    k_drop<<<(d.B + 63) / 64, 64, 0, k->stream>>>(d, dids, cnt, dfound);
    e = hipGetLastError();
  }
  if (e == hipSuccess && found) e = hipMemcpyAsync(found, dfound, n, hipMemcpyDeviceToHost, k->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
  (void)hipFree(dids);
  if (e != hipSuccess) return fail(VIEKF_ERR_HIP, std::string("viekf_klt_drop_features: ") + hipGetErrorString(e));
  return VIEKF_OK;
}

int viekf_klt_sample_depth(viekf_klt* k, const float* depth_mm, double min_depth, double* depth, viekf_mem where) {
  if (!k || !depth_mm || !depth) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(k)) return rc;
  const KltDev& d = k->d;
  const float* src = depth_mm;
  if (where == VIEKF_HOST) {
    if (!k->dimg)
      if (int rc = k->own.alloc(&k->dimg, (size_t)d.B * d.W * d.H)) return rc;
    HIP_TRY(hipMemcpyAsync(k->dimg, depth_mm, sizeof(float) * d.B * d.W * d.H, hipMemcpyHostToDevice, k->stream));
    src = k->dimg;
  }
  k_depth<<<dim3((d.MF + 63) / 64, d.B), 64, 0, k->stream>>>(d, src, min_depth, k->depth);
  HIP_TRY(hipGetLastError());
  if (int rc = copy_out(k, depth, k->depth, sizeof(double) * d.B * d.MF, where)) return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(k->stream));
  return VIEKF_OK;
}

int viekf_klt_get_points(viekf_klt* k, float* pts, int32_t* ids, int32_t* count, int32_t* next_id) {
  if (!k) return fail(VIEKF_ERR_INVALID, "tracker is null");
  if (int rc = set_dev(k)) return rc;
  const KltDev& d = k->d;
  if (int rc = copy_out(k, pts, d.pts, sizeof(float) * d.B * d.MF * 2, VIEKF_HOST)) return rc;
  if (int rc = copy_out(k, ids, d.ids, sizeof(int) * d.B * d.MF, VIEKF_HOST)) return rc;
  if (int rc = copy_out(k, count, d.cnt, sizeof(int) * d.B, VIEKF_HOST)) return rc;
  if (int rc = copy_out(k, next_id, d.next_id, sizeof(int) * d.B, VIEKF_HOST)) return rc;
  HIP_TRY(hipStreamSynchronize(k->stream));
  return VIEKF_OK;
}

int viekf_klt_get_level(viekf_klt* k, int32_t level, uint8_t* out) {
  if (!k || !out) return fail(VIEKF_ERR_INVALID, "null argument");
  if (level < 0 || level >= k->d.nlev) return fail(VIEKF_ERR_INVALID, "level out of range");
  if (int rc = set_dev(k)) return rc;
  const KltDev& d = k->d;
  const size_t n = (size_t)d.lw[level] * d.lh[level];
  uint8_t* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, n * d.B));
  k_get_level<<<dim3((unsigned)((n + 255) / 256), d.B), 256, 0, k->stream>>>(d, level, tmp);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, tmp, n * d.B, hipMemcpyDeviceToHost, k->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(k->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) return fail(VIEKF_ERR_HIP, std::string("viekf_klt_get_level: ") + hipGetErrorString(e));
  return VIEKF_OK;
}

}  // extern "C"
