// viekf_sim.hip -- the batched flight simulator behind include/viekf_sim.h: `batch` vehicles of vi_ekf_amd/sim.py's
// Simulator on the device.  sim.py is the specification: every formula below restates one of its lines
// in double, in its order of operations (this file is compiled without FMA contraction, like the tracker).
//
//   k_sim_step         one lane per vehicle, K ticks in a loop: _control, _step_truth (four sub-steps), imu()
//   k_sim_camera       one workgroup per vehicle: project, visibility window, tracked list, bitonic sort of the
//                      candidates in LDS, pick order cand[::3] + cand[1::3] + cand[2::3], padded outputs
//   k_sim_render       tiles x batch, four horizontally adjacent pixels per thread, landmark table in LDS
//   k_sim_truth_state  the true state in the filter's layout
//
// All synchronisation in this file is __syncthreads(): no flags, tickets or polling between waves.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/viekf_sim.h"
#include "viekf_hostkit.hpp"

namespace {

constexpr double kG = 9.80665;
constexpr int kCamThreads = 256;
constexpr int kTileW = 64, kTileH = 16;           // k_sim_render: 16 x 16 threads, four pixels each along x
constexpr int kStateFields = 14;                  // pos(3) vel(3) q(4) w(3) az, each [B] (structure of arrays)

struct SimDev {
  int B, L, ng, MF, lm_per;
  double dt, acc_sig, gyr_sig, pix_sig, g0, pitch;
  double umin, umax, vmin, vmax, zmin;
  double x0[17];
  double c[2], f[2], qbc[4], pbc[3], qbu[4];
  double* st;                                     // [14][B]
  const unsigned long long* seed;                 // [B]
  const double *radius, *period, *ab, *gb;        // [B], [B], [B][3], [B][3]
  const double* lm;                               // [lm_per ? B : 1][L][3]
  const double* amp;                              // [L]
  int *trk, *tid, *tcnt, *next_id;                // tracked landmark index / feature id [B][MF], count [B], next id [B]
};

#define SD __device__ __forceinline__

SD void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// sim.py q_rotp: passive rotation R(q) v
SD void rotp(const double* q, const double* v, double* o) {
  double c[3], t[3], c2[3];
  cross3(q + 1, v, c);
  for (int i = 0; i < 3; i++) t[i] = -2.0 * c[i];
  cross3(q + 1, t, c2);
  for (int i = 0; i < 3; i++) o[i] = v[i] + q[0] * t[i] - c2[i];
}
// sim.py q_rota: active rotation R(q)^T v
SD void rota(const double* q, const double* v, double* o) {
  double c[3], t[3], c2[3];
  cross3(q + 1, v, c);
  for (int i = 0; i < 3; i++) t[i] = 2.0 * c[i];
  cross3(q + 1, t, c2);
  for (int i = 0; i < 3; i++) o[i] = v[i] + q[0] * t[i] + c2[i];
}
SD double norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
SD double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- noise: Philox4x32-10, two uniforms, Box-Muller (include/viekf_sim.h) ----------------------------------------------
SD void philox4x32_10(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned* o) {
  constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  for (int r = 0; r < 10; r++) {
    const unsigned hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
    const unsigned n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}
SD double uniform53(unsigned hi, unsigned lo) {
  return ((double)(hi >> 5) * 67108864.0 + (double)(lo >> 6) + 0.5) * (1.0 / 9007199254740992.0);
}
SD void normal_pair(unsigned long long seed, long long tick, unsigned stream, unsigned block, double* n0, double* n1) {
  unsigned w[4];
  philox4x32_10((unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)(unsigned long long)tick, stream, block, 0u, w);
  const double u1 = uniform53(w[0], w[1]), u2 = uniform53(w[2], w[3]);
  const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
  *n0 = r * cos(a);
  *n1 = r * sin(a);
}

// ---- truth and IMU -------------------------------------------------------------------------------------------------------
struct Veh { double pos[3], vel[3], q[4], w[3], az; };

SD void veh_load(const SimDev& d, int b, Veh& v) {
  const double* s = d.st + b;
  for (int i = 0; i < 3; i++) v.pos[i] = s[(long long)i * d.B];
  for (int i = 0; i < 3; i++) v.vel[i] = s[(long long)(3 + i) * d.B];
  for (int i = 0; i < 4; i++) v.q[i] = s[(long long)(6 + i) * d.B];
  for (int i = 0; i < 3; i++) v.w[i] = s[(long long)(10 + i) * d.B];
  v.az = s[13ll * d.B];
}
SD void veh_store(const SimDev& d, int b, const Veh& v) {
  double* s = d.st + b;
  for (int i = 0; i < 3; i++) s[(long long)i * d.B] = v.pos[i];
  for (int i = 0; i < 3; i++) s[(long long)(3 + i) * d.B] = v.vel[i];
  for (int i = 0; i < 4; i++) s[(long long)(6 + i) * d.B] = v.q[i];
  for (int i = 0; i < 3; i++) s[(long long)(10 + i) * d.B] = v.w[i];
  s[13ll * d.B] = v.az;
}

// Simulator.commanded + _control at time t
SD void control(const SimDev& d, Veh& v, double t, double radius, double period) {
  const double a = 2.0 * M_PI * t / period;
  const double ramp = fmin(1.0, t / 2.0);
  const double pc[3] = {d.x0[0] + ramp * (radius * (cos(a) - 1.0)), d.x0[1] + ramp * (radius * sin(a)),
                        d.x0[2] + ramp * (-0.3 * sin(0.5 * a))};
  const double yaw_c = 0.25 * ramp * sin(0.7 * a);
  double v_i[3], f_i[3], nf[3], zb[3];
  rota(v.q, v.vel, v_i);
  for (int i = 0; i < 3; i++) f_i[i] = clip(2.0 * (pc[i] - v.pos[i]) - 2.5 * v_i[i], -2.0, 2.0);
  f_i[2] = f_i[2] - kG;
  const double thrust = norm3(f_i);
  for (int i = 0; i < 3; i++) nf[i] = -f_i[i] / thrust;
  rotp(v.q, nf, zb);
  const double axis[3] = {0.0 * zb[2] - 1.0 * zb[1], 1.0 * zb[0] - 0.0 * zb[2], 0.0};
  const double s = norm3(axis);
  const double ang = atan2(s, zb[2]);
  double wx = 0.0, wy = 0.0;
  if (s > 1e-12) { wx = 6.0 * ang * axis[0] / s; wy = 6.0 * ang * axis[1] / s; }
  const double ex[3] = {1.0, 0.0, 0.0};
  double xb[3];
  rota(v.q, ex, xb);
  const double yaw = atan2(xb[1], xb[0]);
  v.w[0] = clip(wx, -1.5, 1.5);
  v.w[1] = clip(wy, -1.5, 1.5);
  v.w[2] = clip(2.0 * (yaw_c - yaw), -1.5, 1.5);
  v.az = -thrust;
}

// Simulator._step_truth: four sub-steps of one IMU period
SD void step_truth(const SimDev& d, Veh& v) {
  const double h = d.dt / 4, mu = d.x0[16];
  const double gz[3] = {0.0, 0.0, kG};
  for (int it = 0; it < 4; it++) {
    double gB[3], wxv[3], vi[3], vdot[3];
    rotp(v.q, gz, gB);
    cross3(v.w, v.vel, wxv);
    vdot[0] = 0.0 + gB[0] - wxv[0] - mu * v.vel[0];
    vdot[1] = 0.0 + gB[1] - wxv[1] - mu * v.vel[1];
    vdot[2] = v.az + gB[2] - wxv[2] - mu * 0.0;
    rota(v.q, v.vel, vi);
    for (int i = 0; i < 3; i++) v.pos[i] = v.pos[i] + h * vi[i];
    for (int i = 0; i < 3; i++) v.vel[i] = v.vel[i] + h * vdot[i];
    // q_exp(h w)
    const double r[3] = {h * v.w[0], h * v.w[1], h * v.w[2]};
    const double th = norm3(r);
    double e[4];
    if (th < 1e-9) {
      e[0] = 1.0; e[1] = 0.5 * r[0]; e[2] = 0.5 * r[1]; e[3] = 0.5 * r[2];
    } else {
      const double sn = sin(th / 2);
      e[0] = cos(th / 2); e[1] = sn * r[0] / th; e[2] = sn * r[1] / th; e[3] = sn * r[2] / th;
    }
    const double ne = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2] + e[3] * e[3]);
    for (int i = 0; i < 4; i++) e[i] = e[i] / ne;
    // q_otimes(q, e), then normalise
    double c[3], qn[4];
    cross3(v.q + 1, e + 1, c);
    qn[0] = v.q[0] * e[0] - (v.q[1] * e[1] + v.q[2] * e[2] + v.q[3] * e[3]);
    for (int i = 0; i < 3; i++) qn[1 + i] = v.q[0] * e[1 + i] + e[0] * v.q[1 + i] + c[i];
    const double nq = sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
    for (int i = 0; i < 4; i++) v.q[i] = qn[i] / nq;
  }
}

// Simulator.imu() at tick k
SD void imu_sample(const SimDev& d, const Veh& v, int b, long long k, const double* ab, const double* gb, unsigned long long seed,
                   double* u) {
  const double mu = d.x0[16];
  double n[6];
  normal_pair(seed, k, 0u, 0u, n + 0, n + 1);
  normal_pair(seed, k, 0u, 1u, n + 2, n + 3);
  normal_pair(seed, k, 0u, 2u, n + 4, n + 5);
  double acc[3] = {-mu * v.vel[0] + ab[0], -mu * v.vel[1] + ab[1], v.az + ab[2]};
  double gyr[3] = {v.w[0] + gb[0], v.w[1] + gb[1], v.w[2] + gb[2]};
  for (int i = 0; i < 3; i++) { acc[i] = acc[i] + d.acc_sig * n[i]; gyr[i] = gyr[i] + d.gyr_sig * n[3 + i]; }
  rotp(d.qbu, acc, u);
  rotp(d.qbu, gyr, u + 3);
}

// mode 0: K ticks from tick k0, u [K][B][6].  mode 1: the constructor's _control() at t = 0 (no output).
// mode 2: imu() at tick k0 without stepping, u [B][6].
__global__ __launch_bounds__(64) void k_sim_step(SimDev d, long long k0, int K, int mode, double* __restrict__ u) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= d.B) return;
  Veh v;
  veh_load(d, b, v);
  const double radius = d.radius[b], period = d.period[b];
  const double ab[3] = {d.ab[3ll * b], d.ab[3ll * b + 1], d.ab[3ll * b + 2]};
  const double gb[3] = {d.gb[3ll * b], d.gb[3ll * b + 1], d.gb[3ll * b + 2]};
  const unsigned long long seed = d.seed[b];
  if (mode == 1) {
    control(d, v, 0.0, radius, period);
    veh_store(d, b, v);
    return;
  }
  if (mode == 2) {
    double s[6];
    imu_sample(d, v, b, k0, ab, gb, seed, s);
    double2* o = reinterpret_cast<double2*>(u + 6ll * b);
    o[0] = make_double2(s[0], s[1]); o[1] = make_double2(s[2], s[3]); o[2] = make_double2(s[4], s[5]);
    return;
  }
  for (int i = 0; i < K; i++) {
    const long long k = k0 + i;
    control(d, v, (double)k * d.dt, radius, period);
    step_truth(d, v);
    double s[6];
    imu_sample(d, v, b, k + 1, ab, gb, seed, s);
    // lane b writes 48 contiguous bytes next to lane b + 1's: one wave covers a contiguous 3 KiB of u[k]
    double2* o = reinterpret_cast<double2*>(u + ((long long)i * d.B + b) * 6);
    o[0] = make_double2(s[0], s[1]); o[1] = make_double2(s[2], s[3]); o[2] = make_double2(s[4], s[5]);
  }
  veh_store(d, b, v);
}

// ---- camera --------------------------------------------------------------------------------------------------------------
// Simulator.project for one landmark: pixel, range |p_c| and the visibility window
SD bool project(const SimDev& d, const Veh& v, const double* l, double* pix, double* range, double* pc_out) {
  double dl[3] = {l[0] - v.pos[0], l[1] - v.pos[1], l[2] - v.pos[2]}, pb[3], pc[3];
  rotp(v.q, dl, pb);
  for (int i = 0; i < 3; i++) pb[i] = pb[i] - d.pbc[i];
  rotp(d.qbc, pb, pc);
  const bool ok = pc[2] > d.zmin;
  const double zs = ok ? pc[2] : 1.0;
  pix[0] = d.f[0] * pc[0] / zs + d.c[0];
  pix[1] = d.f[1] * pc[1] / zs + d.c[1];
  *range = norm3(pc);
  if (pc_out) { pc_out[0] = pc[0]; pc_out[1] = pc[1]; pc_out[2] = pc[2]; }
  return ok && pix[0] > d.umin && pix[0] < d.umax && pix[1] > d.vmin && pix[1] < d.vmax;
}

__global__ __launch_bounds__(kCamThreads) void k_sim_camera(SimDev d, long long tick, int N, double* __restrict__ z,
                                                            int* __restrict__ ids, int* __restrict__ count,
                                                            double* __restrict__ depth, int* __restrict__ landmark) {
  constexpr int LP = VIEKF_SIM_MAX_LANDMARKS;
  __shared__ double px[LP], py[LP], rg[LP];
  __shared__ unsigned long long key[LP];          // distance bits (a non-negative double orders as its bits)
  __shared__ unsigned short idx[LP];
  __shared__ unsigned char vis[LP], tracked[LP];
  __shared__ int s_cnt, s_ncand, s_nid;
  const int b = blockIdx.x, tid = threadIdx.x, L = d.L;
  Veh v;
  veh_load(d, b, v);
  const double* lm = d.lm + (d.lm_per ? (long long)b * L * 3 : 0ll);
  int np2 = 1;
  while (np2 < L) np2 <<= 1;
  for (int l = tid; l < np2; l += kCamThreads) {
    bool ok = false;
    double dist = 0.0;
    if (l < L) {
      double pix[2], r;
      ok = project(d, v, lm + 3ll * l, pix, &r, nullptr);
      px[l] = pix[0]; py[l] = pix[1]; rg[l] = r;
      const double ex = pix[0] - d.c[0], ey = pix[1] - d.c[1];
      dist = sqrt(ex * ex + ey * ey);
      vis[l] = ok;
      tracked[l] = 0;
    }
    key[l] = ok ? (unsigned long long)__double_as_longlong(dist) : ~0ull;
    idx[l] = (unsigned short)l;
  }
  __syncthreads();
  // the tracked list, in order: drop what left the window (its id is forgotten), cut to the capacity
  int* trk = d.trk + (long long)b * d.MF;
  int* fid = d.tid + (long long)b * d.MF;
  if (tid == 0) {
    const int n0 = d.tcnt[b];
    int n = 0;
    for (int i = 0; i < n0 && n < N; i++) {
      const int l = trk[i];
      if (vis[l]) { trk[n] = l; fid[n] = fid[i]; tracked[l] = 1; n++; }
    }
    s_cnt = n;
    s_nid = d.next_id[b];
  }
  __syncthreads();
  for (int l = tid; l < L; l += kCamThreads)
    if (tracked[l]) key[l] = ~0ull;               // (before the sort idx[l] == l)
  __syncthreads();
  // bitonic sort of (distance bits, landmark index), ascending; what is not a candidate sorts to the end
  for (int k = 2; k <= np2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < np2; t += kCamThreads) {
        const int p = t ^ j;
        if (p > t) {
          const unsigned long long a = key[t], c = key[p];
          const unsigned short ia = idx[t], ic = idx[p];
          const bool gt = a > c || (a == c && ia > ic);
          if (gt == ((t & k) == 0)) { key[t] = c; key[p] = a; idx[t] = ic; idx[p] = ia; }
        }
      }
      __syncthreads();
    }
  }
  // candidates are now the leading entries: count them (block-wide sum in LDS, no atomics between waves)
  if (tid == 0) s_ncand = 0;
  __syncthreads();
  int mine = 0;
  for (int t = tid; t < np2; t += kCamThreads) mine += key[t] != ~0ull;
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o, 64);
  __shared__ int wsum[kCamThreads / 64];
  if ((tid & 63) == 0) wsum[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int i = 0; i < kCamThreads / 64; i++) s += wsum[i];
    s_ncand = s;
  }
  __syncthreads();
  const int cnt0 = s_cnt, ncand = s_ncand, nid = s_nid;
  const int need = N - cnt0 > 0 ? N - cnt0 : 0;
  const int take = need < ncand ? need : ncand;
  // rank r in distance order -> its place in cand[::3] + cand[1::3] + cand[2::3]
  const int n0 = (ncand + 2) / 3, n1 = (ncand + 1) / 3;
  for (int r = tid; r < ncand; r += kCamThreads) {
    const int m = r % 3;
    const int pos = r / 3 + (m == 0 ? 0 : (m == 1 ? n0 : n0 + n1));
    if (pos < take) { trk[cnt0 + pos] = idx[r]; fid[cnt0 + pos] = nid + pos; }
  }
  __syncthreads();
  const int total = cnt0 + take;
  const unsigned long long seed = d.seed[b];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int j = tid; j < N; j += kCamThreads) {
    double zx = nan, zy = nan, dp = nan;
    int id = -1, l = -1;
    if (j < total) {
      l = trk[j];
      id = fid[j];
      double n0x, n1y;
      normal_pair(seed, tick, 1u, (unsigned)l, &n0x, &n1y);
      zx = px[l] + d.pix_sig * n0x;
      zy = py[l] + d.pix_sig * n1y;
      dp = rg[l];
    }
    const long long o = (long long)b * N + j;
    z[2 * o] = zx; z[2 * o + 1] = zy;
    ids[o] = id;
    if (depth) depth[o] = dp;
    if (landmark) landmark[o] = l;
  }
  if (tid == 0) {
    d.tcnt[b] = total;
    d.next_id[b] = nid + take;
    count[b] = total;
  }
}

// ---- render ---------------------------------------------------------------------------------------------------------------
// Simulator.render for one pixel: the value before rint / clip, and the range in mm
SD void shade_pixel(const SimDev& d, const double* R, const double* C, const double* lmx, const double* lmy, const double* amp,
                    double u, double v, double* grey, float* mm) {
  const double dc0 = (u - d.c[0]) / d.f[0], dc1 = (v - d.c[1]) / d.f[1];
  const double d0 = dc0 * R[0] + dc1 * R[1] + R[2], d1 = dc0 * R[3] + dc1 * R[4] + R[5], d2 = dc0 * R[6] + dc1 * R[7] + R[8];
  double t = -C[2] / d2;
  const bool hit = isfinite(t) && t > 0.0;
  if (!hit) {                                     // (a whole tile above the horizon leaves here together)
    *grey = 30.0;
    *mm = __int_as_float(0x7f800000);
    return;
  }
  const double X = C[0] + t * d0, Y = C[1] + t * d1;
  const double fi = floor((X - d.g0) / d.pitch), fj = floor((Y - d.g0) / d.pitch);
  double blobs = 0.0;
  for (int di = 0; di < 2; di++)
    for (int dj = 0; dj < 2; dj++) {
      const double i = fi + di, j = fj + dj;
      if (i >= 0.0 && i < d.ng && j >= 0.0 && j < d.ng) {      // (tested in double: a grazing ray's X does not fit an int)
        const int k = (int)i * d.ng + (int)j;
        const double ex = X - lmx[k], ey = Y - lmy[k];
        const double r2 = ex * ex + ey * ey;
        blobs += amp[k] * exp(-r2 * (1.0 / (2 * 0.045 * 0.045)));
      }
    }
  const double shade = 0.5 + 0.25 * sin(1.3 * X + 0.4) * cos(0.9 * Y - 0.2);
  *grey = 50.0 + 60.0 * shade + 140.0 * fmin(blobs, 1.0);
  *mm = (float)(t * sqrt(d0 * d0 + d1 * d1 + d2 * d2) * 1e3);
}

SD unsigned grey_byte(double g) {
  const double r = rint(g);
  return (unsigned)(r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r));   // (a NaN gives 0)
}

__global__ __launch_bounds__(256) void k_sim_render(SimDev d, int W, int H, int tiles_x, uint8_t* __restrict__ img,
                                                    float* __restrict__ dmm) {
  __shared__ double lmx[VIEKF_SIM_MAX_LANDMARKS], lmy[VIEKF_SIM_MAX_LANDMARKS], amp[VIEKF_SIM_MAX_LANDMARKS];
  __shared__ double RC[12];                       // camera -> inertial, row-major, then the camera centre
  const int b = blockIdx.y, tid = threadIdx.x;
  const double* lm = d.lm + (d.lm_per ? (long long)b * d.L * 3 : 0ll);
  for (int l = tid; l < d.L; l += 256) { lmx[l] = lm[3ll * l]; lmy[l] = lm[3ll * l + 1]; amp[l] = d.amp[l]; }
  if (tid == 0) {
    Veh v;
    veh_load(d, b, v);
    double Rbc[9], Rib[9];                        // columns rota(q, e_i), stored row-major
    for (int i = 0; i < 3; i++) {
      const double e[3] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0};
      double c[3];
      rota(d.qbc, e, c);
      Rbc[i] = c[0]; Rbc[3 + i] = c[1]; Rbc[6 + i] = c[2];
      rota(v.q, e, c);
      Rib[i] = c[0]; Rib[3 + i] = c[1]; Rib[6 + i] = c[2];
    }
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) RC[3 * r + c] = Rib[3 * r] * Rbc[c] + Rib[3 * r + 1] * Rbc[3 + c] + Rib[3 * r + 2] * Rbc[6 + c];
    double o[3];
    rota(v.q, d.pbc, o);
    for (int i = 0; i < 3; i++) RC[9 + i] = v.pos[i] + o[i];
  }
  __syncthreads();
  const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
  const int x0 = tile_x * kTileW + (tid & 15) * 4, y = tile_y * kTileH + (tid >> 4);
  if (y >= H || x0 >= W) return;                  // (after the only barrier)
  double g[4];
  float m[4];
  for (int i = 0; i < 4; i++) {
    g[i] = 30.0; m[i] = 0.f;
    if (x0 + i < W) shade_pixel(d, RC, RC + 9, lmx, lmy, amp, (double)(x0 + i), (double)y, &g[i], &m[i]);
  }
  const unsigned q0 = grey_byte(g[0]), q1 = grey_byte(g[1]), q2 = grey_byte(g[2]), q3 = grey_byte(g[3]);
  const long long a = ((long long)b * H + y) * W + x0;
  if ((W & 3) == 0) {                             // whole groups: one 32-bit word of grey, one 16-byte vector of depth
    *reinterpret_cast<unsigned*>(img + a) = q0 | (q1 << 8) | (q2 << 16) | (q3 << 24);
    if (dmm) *reinterpret_cast<float4*>(dmm + a) = make_float4(m[0], m[1], m[2], m[3]);
  } else {                                        // W even: pairs (every row starts on a pair; a pair is inside or outside)
    *reinterpret_cast<unsigned short*>(img + a) = (unsigned short)(q0 | (q1 << 8));
    if (dmm) *reinterpret_cast<float2*>(dmm + a) = make_float2(m[0], m[1]);
    if (x0 + 2 < W) {
      *reinterpret_cast<unsigned short*>(img + a + 2) = (unsigned short)(q2 | (q3 << 8));
      if (dmm) *reinterpret_cast<float2*>(dmm + a + 2) = make_float2(m[2], m[3]);
    }
  }
}

// ---- truth ----------------------------------------------------------------------------------------------------------------
__global__ void k_sim_get_truth(SimDev d, long long tick, double* __restrict__ state, double* __restrict__ t) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= d.B) return;
  if (state) {
    Veh v;
    veh_load(d, b, v);
    double* o = state + 13ll * b;
    for (int i = 0; i < 3; i++) o[i] = v.pos[i];
    for (int i = 0; i < 4; i++) o[3 + i] = v.q[i];
    for (int i = 0; i < 3; i++) o[7 + i] = v.vel[i];
    for (int i = 0; i < 3; i++) o[10 + i] = v.w[i];
  }
  if (t) t[b] = (double)tick * d.dt;
}

// thread (b, j): j < N a feature slot, j == N the body part
__global__ __launch_bounds__(64) void k_sim_truth_state(SimDev d, const int* __restrict__ ids, int N, double* __restrict__ x) {
  const int b = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
  if (j > N) return;
  Veh v;
  veh_load(d, b, v);
  double* xb = x + (long long)b * (17 + 5 * N);
  if (j == N) {
    for (int i = 0; i < 3; i++) xb[i] = v.pos[i];
    for (int i = 0; i < 3; i++) xb[3 + i] = v.vel[i];
    for (int i = 0; i < 4; i++) xb[6 + i] = v.q[i];
    for (int i = 0; i < 3; i++) xb[10 + i] = d.ab[3ll * b + i];
    for (int i = 0; i < 3; i++) xb[13 + i] = d.gb[3ll * b + i];
    xb[16] = d.x0[16];
    return;
  }
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double o[5] = {nan, nan, nan, nan, nan};
  const int id = ids[(long long)b * N + j];
  int l = -1;
  if (id >= 0) {
    const int n = d.tcnt[b];
    for (int i = 0; i < n; i++)
      if (d.tid[(long long)b * d.MF + i] == id) { l = d.trk[(long long)b * d.MF + i]; break; }
  }
  if (l >= 0) {
    const double* lm = d.lm + (d.lm_per ? (long long)b * d.L * 3 : 0ll) + 3ll * l;
    double pix[2], r, pc[3];
    (void)project(d, v, lm, pix, &r, pc);
    const double zt[3] = {pc[0] / r, pc[1] / r, pc[2] / r};
    // from_two_unit_vectors(e_z, zeta) (reference src/quat.cpp:167-185), as init_feature_state has it
    const double dd = zt[2];
    if (dd < 1.0) {
      const double invs = 1.0 / sqrt(2.0 * (1.0 + dd));
      const double qq[4] = {0.5 / invs, -zt[1] * invs, zt[0] * invs, 0.0};
      const double nq = sqrt(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
      for (int i = 0; i < 4; i++) o[i] = qq[i] / nq;
    } else {
      o[0] = 1.0; o[1] = 0.0; o[2] = 0.0; o[3] = 0.0;
    }
    o[4] = 1.0 / r;
  }
  for (int i = 0; i < 5; i++) xb[17 + 5 * j + i] = o[i];
}

__global__ void k_sim_amp(double* amp, int L) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < L) amp[k] = 0.55 + 0.45 * sin(12.9898 * k + 4.1414);
}

// every vehicle to x0 with nothing tracked (the constructor's _control() follows as k_sim_step mode 1)
__global__ void k_sim_init(SimDev d) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= d.B) return;
  Veh v;
  for (int i = 0; i < 3; i++) { v.pos[i] = d.x0[i]; v.vel[i] = d.x0[3 + i]; v.w[i] = 0.0; }
  for (int i = 0; i < 4; i++) v.q[i] = d.x0[6 + i];
  v.az = -kG;
  veh_store(d, b, v);
  d.tcnt[b] = 0;
  d.next_id[b] = 0;
}

}  // namespace

struct viekf_sim {
  SimDev d{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  DevOwner own;                                   // every device buffer below
  long long tick = 0;
  // per-vehicle values and the landmark field (owned; SimDev holds const views of them)
  unsigned long long* seed = nullptr;
  double *radius = nullptr, *period = nullptr, *ab = nullptr, *gb = nullptr, *lm = nullptr, *amp = nullptr;
  size_t lm_count = 0;                            // capacity of lm in doubles: one field until a per-vehicle one is set
  // growable device staging for callers with host pointers (bytes)
  char* stage[2] = {nullptr, nullptr};
  size_t stage_sz[2] = {0, 0};
};

namespace {

// the end of a simulator (the caller has set the device and waited for its stream)
void sim_delete(viekf_sim* s) {
  s->own.release_all();
  if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

// device staging buffer `i` of at least `bytes` (for callers with host pointers)
template <class T>
int sim_stage(viekf_sim* s, int i, size_t bytes, T** out) {
  if (int rc = s->own.reserve(&s->stage[i], &s->stage_sz[i], bytes, s->stream)) return rc;
  *out = reinterpret_cast<T*>(s->stage[i]);
  return VIEKF_OK;
}

int copy_out(viekf_sim* s, void* dst, const void* src, size_t bytes, viekf_mem where) {
  return copy_user(dst, src, bytes, where, Copy::ToUser, s->stream);
}

int copy_in(viekf_sim* s, void* dst, const void* src, size_t bytes, viekf_mem where) {
  return copy_user(dst, src, bytes, where, Copy::FromUser, s->stream);
}

int set_dev(const viekf_sim* s) {
  HIP_TRY(hipSetDevice(s->device));
  return VIEKF_OK;
}

// x0, tick 0, nothing tracked, then the constructor's _control()
int sim_restart(viekf_sim* s) {
  const unsigned g = (unsigned)((s->d.B + 63) / 64);
  k_sim_init<<<g, 64, 0, s->stream>>>(s->d);
  k_sim_step<<<g, 64, 0, s->stream>>>(s->d, 0ll, 0, 1, nullptr);
  HIP_TRY(hipGetLastError());
  s->tick = 0;
  return VIEKF_OK;
}

}  // namespace

extern "C" {

int viekf_sim_config_default(viekf_sim_config* c) {
  if (!c) return fail(VIEKF_ERR_INVALID, "config is null");
  std::memset(c, 0, sizeof(*c));
  c->imu_rate = 250.0;
  c->accel_sigma = 0.3; c->gyro_sigma = 0.01; c->pix_sigma = 0.5;
  c->grid_origin = -3.0; c->grid_pitch = 0.22; c->grid_n = 28;
  c->max_features = 12;
  c->win_u_min = 15.0; c->win_u_max = 625.0; c->win_v_min = 15.0; c->win_v_max = 465.0;
  c->win_min_depth = 0.2;
  return VIEKF_OK;
}

int viekf_sim_create(int32_t batch, const viekf_params* p, const viekf_sim_config* c, int32_t device, viekf_sim** out) {
  if (!out) return fail(VIEKF_ERR_INVALID, "out is null");
  *out = nullptr;
  if (!p || !c) return fail(VIEKF_ERR_INVALID, "params or config is null");
  if (batch <= 0 || batch > 65535) return fail(VIEKF_ERR_INVALID, "batch must be in [1, 65535]");
  if (c->grid_n < 1 || (long long)c->grid_n * c->grid_n > VIEKF_SIM_MAX_LANDMARKS)
    return fail(VIEKF_ERR_INVALID, "grid_n^2 landmarks must be in [1, 1024]");
  if (c->max_features < 1 || c->max_features > VIEKF_SIM_MAX_LANDMARKS) return fail(VIEKF_ERR_INVALID, "max_features must be in [1, 1024]");
  if (!(c->imu_rate > 0.0) || !(c->grid_pitch > 0.0)) return fail(VIEKF_ERR_INVALID, "imu_rate and grid_pitch must be > 0");
  if (!(c->accel_sigma >= 0.0) || !(c->gyro_sigma >= 0.0) || !(c->pix_sigma >= 0.0)) return fail(VIEKF_ERR_INVALID, "sigmas must be >= 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    (void)hipGetLastError();
    return fail(VIEKF_ERR_NO_DEVICE, "no HIP device available (this library has no CPU path)");
  }
  if (device < 0 || device >= ndev) return fail(VIEKF_ERR_NO_DEVICE, "device index out of range");
  HIP_TRY(hipSetDevice(device));
  viekf_sim* s = new (std::nothrow) viekf_sim();
  if (!s) return fail(VIEKF_ERR_HIP, "out of host memory");
  s->device = device;
  SimDev& d = s->d;
  d.B = batch; d.ng = c->grid_n; d.L = c->grid_n * c->grid_n; d.MF = c->max_features; d.lm_per = 0;
  d.dt = 1.0 / c->imu_rate;
  d.acc_sig = c->accel_sigma; d.gyr_sig = c->gyro_sigma; d.pix_sig = c->pix_sigma;
  d.g0 = c->grid_origin; d.pitch = c->grid_pitch;
  d.umin = c->win_u_min; d.umax = c->win_u_max; d.vmin = c->win_v_min; d.vmax = c->win_v_max; d.zmin = c->win_min_depth;
  for (int i = 0; i < 17; i++) d.x0[i] = p->x0[i];
  for (int i = 0; i < 2; i++) { d.c[i] = p->cam_center[i]; d.f[i] = p->focal_len[i]; }
  for (int i = 0; i < 4; i++) { d.qbc[i] = p->q_b_c[i]; d.qbu[i] = p->q_b_u[i]; }
  for (int i = 0; i < 3; i++) d.pbc[i] = p->p_b_c[i];
  int rc = VIEKF_OK;
  auto fin = [&](int code) { sim_delete(s); return code; };
  if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) return fin(fail(VIEKF_ERR_HIP, "hipStreamCreate failed"));
  s->own_stream = true;
  const size_t B = batch, MF = d.MF, L = d.L;
  auto zeroed = [&](auto** p, size_t count) { return s->own.alloc_zeroed(p, count, s->stream); };
  if ((rc = zeroed(&d.st, kStateFields * B)) || (rc = zeroed(&s->seed, B)) || (rc = zeroed(&s->radius, B)) ||
      (rc = zeroed(&s->period, B)) || (rc = zeroed(&s->ab, 3 * B)) || (rc = zeroed(&s->gb, 3 * B)) ||
      (rc = zeroed(&s->amp, L)) || (rc = zeroed(&d.trk, B * MF)) ||
      (rc = zeroed(&d.tid, B * MF)) || (rc = zeroed(&d.tcnt, B)) || (rc = zeroed(&d.next_id, B)))
    return fin(rc);
  if (s->own.alloc(&s->lm, 3 * L)) return fin(fail(VIEKF_ERR_HIP, "hipMalloc of the landmark field failed"));
  s->lm_count = 3 * L;
  d.seed = s->seed; d.radius = s->radius; d.period = s->period; d.ab = s->ab; d.gb = s->gb; d.lm = s->lm; d.amp = s->amp;
  // defaults: sim.py's per-vehicle values, the regular grid (after the allocations' clears, which run on the stream)
  if (hipStreamSynchronize(s->stream) != hipSuccess) return fin(fail(VIEKF_ERR_HIP, "clearing the simulator's buffers failed"));
  {
    unsigned long long* hs = new (std::nothrow) unsigned long long[B];
    double* hv = new (std::nothrow) double[3 * B > 3 * L ? 3 * B : 3 * L];
    if (!hs || !hv) {
      delete[] hs;
      delete[] hv;
      return fin(fail(VIEKF_ERR_HIP, "out of host memory"));
    }
    bool ok = true;
    for (size_t b = 0; b < B; b++) hs[b] = b + 1;
    ok = ok && hipMemcpy(s->seed, hs, 8 * B, hipMemcpyHostToDevice) == hipSuccess;
    for (size_t b = 0; b < B; b++) hv[b] = 0.35;
    ok = ok && hipMemcpy(s->radius, hv, 8 * B, hipMemcpyHostToDevice) == hipSuccess;
    for (size_t b = 0; b < B; b++) hv[b] = 8.0;
    ok = ok && hipMemcpy(s->period, hv, 8 * B, hipMemcpyHostToDevice) == hipSuccess;
    for (size_t b = 0; b < B; b++) { hv[3 * b] = 0.05; hv[3 * b + 1] = -0.04; hv[3 * b + 2] = 0.03; }
    ok = ok && hipMemcpy(s->ab, hv, 24 * B, hipMemcpyHostToDevice) == hipSuccess;
    for (size_t b = 0; b < B; b++) { hv[3 * b] = 0.004; hv[3 * b + 1] = -0.003; hv[3 * b + 2] = 0.002; }
    ok = ok && hipMemcpy(s->gb, hv, 24 * B, hipMemcpyHostToDevice) == hipSuccess;
    for (int i = 0; i < d.ng; i++)
      for (int j = 0; j < d.ng; j++) {
        double* l = hv + 3 * ((size_t)i * d.ng + j);
        l[0] = d.g0 + i * d.pitch; l[1] = d.g0 + j * d.pitch; l[2] = 0.0;
      }
    ok = ok && hipMemcpy(s->lm, hv, 24 * L, hipMemcpyHostToDevice) == hipSuccess;
    delete[] hs;
    delete[] hv;
    if (!ok) return fin(fail(VIEKF_ERR_HIP, "initialising the simulator's buffers failed"));
  }
  k_sim_amp<<<(unsigned)((L + 255) / 256), 256, 0, s->stream>>>(s->amp, d.L);
  if (sim_restart(s) != VIEKF_OK || hipStreamSynchronize(s->stream) != hipSuccess) return fin(fail(VIEKF_ERR_HIP, "simulator setup failed"));
  *out = s;
  return VIEKF_OK;
}

int viekf_sim_destroy(viekf_sim* s) {
  if (!s) return fail(VIEKF_ERR_INVALID, "simulator is null");
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  sim_delete(s);
  return VIEKF_OK;
}

int viekf_sim_dims(const viekf_sim* s, int32_t* batch, int32_t* landmarks, int32_t* max_features, int64_t* tick) {
  if (!s) return fail(VIEKF_ERR_INVALID, "simulator is null");
  if (batch) *batch = s->d.B;
  if (landmarks) *landmarks = s->d.L;
  if (max_features) *max_features = s->d.MF;
  if (tick) *tick = s->tick;
  return VIEKF_OK;
}

int viekf_sim_reset(viekf_sim* s) {
  if (!s) return fail(VIEKF_ERR_INVALID, "simulator is null");
  if (int rc = set_dev(s)) return rc;
  if (int rc = sim_restart(s)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return VIEKF_OK;
}

int viekf_sim_set_stream(viekf_sim* s, void* hip_stream) {
  if (!s) return fail(VIEKF_ERR_INVALID, "simulator is null");
  if (int rc = set_dev(s)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (s->own_stream) HIP_TRY(hipStreamDestroy(s->stream));
  s->own_stream = false;
  s->stream = static_cast<hipStream_t>(hip_stream);
  return VIEKF_OK;
}

int viekf_sim_sync(viekf_sim* s) {
  if (!s) return fail(VIEKF_ERR_INVALID, "simulator is null");
  if (int rc = set_dev(s)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return VIEKF_OK;
}

int viekf_sim_set_vehicles(viekf_sim* s, const uint64_t* seed, const double* radius, const double* period, const double* accel_bias,
                           const double* gyro_bias, viekf_mem where) {
  if (!s) return fail(VIEKF_ERR_INVALID, "simulator is null");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(s)) return rc;
  const size_t B = s->d.B;
  if (period && where == VIEKF_HOST)
    for (size_t b = 0; b < B; b++)
      if (!(period[b] > 0.0)) return fail(VIEKF_ERR_INVALID, "period must be > 0");
  int rc;
  if ((rc = copy_in(s, s->seed, seed, 8 * B, where)) || (rc = copy_in(s, s->radius, radius, 8 * B, where)) ||
      (rc = copy_in(s, s->period, period, 8 * B, where)) || (rc = copy_in(s, s->ab, accel_bias, 24 * B, where)) ||
      (rc = copy_in(s, s->gb, gyro_bias, 24 * B, where)) || (rc = sim_restart(s)))
    return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(s->stream));
  return VIEKF_OK;
}

int viekf_sim_set_landmarks(viekf_sim* s, const double* lm, int32_t per_vehicle, viekf_mem where) {
  if (!s || !lm) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(s)) return rc;
  SimDev& d = s->d;
  const size_t n = (per_vehicle ? (size_t)d.B : 1) * d.L * 3;
  if (s->lm_count < n) {                          // the first per-vehicle field: room for one field per vehicle
    HIP_TRY(hipStreamSynchronize(s->stream));
    double* q = nullptr;                          // (the old field stays if this fails: alloc, then free)
    if (int rc = s->own.alloc(&q, n)) return rc;
    (void)s->own.free(&s->lm);
    s->lm = q;
    s->lm_count = n;
    d.lm = q;
  }
  if (int rc = copy_in(s, s->lm, lm, 8 * n, where)) return rc;
  d.lm_per = per_vehicle != 0;
  k_sim_amp<<<(unsigned)((d.L + 255) / 256), 256, 0, s->stream>>>(s->amp, d.L);
  if (int rc = sim_restart(s)) return rc;
  if (where == VIEKF_HOST) HIP_TRY(hipStreamSynchronize(s->stream));
  return VIEKF_OK;
}

int viekf_sim_imu(viekf_sim* s, double* u, viekf_mem where) {
  if (!s || !u) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && (reinterpret_cast<uintptr_t>(u) & 15)) return fail(VIEKF_ERR_INVALID, "u must be 16-byte aligned");
  if (int rc = set_dev(s)) return rc;
  const size_t bytes = 48 * (size_t)s->d.B;
  double* du = u;
  if (where == VIEKF_HOST)
    if (int rc = sim_stage(s, 0, bytes, &du)) return rc;
  k_sim_step<<<(unsigned)((s->d.B + 63) / 64), 64, 0, s->stream>>>(s->d, s->tick, 0, 2, du);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    if (int rc = copy_out(s, u, du, bytes, where)) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return VIEKF_OK;
}

int viekf_sim_step(viekf_sim* s, int32_t K, double* u, viekf_mem where) {
  if (!s || !u) return fail(VIEKF_ERR_INVALID, "null argument");
  if (K < 1 || K > (1 << 20)) return fail(VIEKF_ERR_INVALID, "K must be in [1, 2^20]");
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && (reinterpret_cast<uintptr_t>(u) & 15)) return fail(VIEKF_ERR_INVALID, "u must be 16-byte aligned");
  if (int rc = set_dev(s)) return rc;
  const size_t bytes = 48 * (size_t)s->d.B * K;
  double* du = u;
  if (where == VIEKF_HOST)
    if (int rc = sim_stage(s, 0, bytes, &du)) return rc;
  k_sim_step<<<(unsigned)((s->d.B + 63) / 64), 64, 0, s->stream>>>(s->d, s->tick, K, 0, du);
  HIP_TRY(hipGetLastError());
  s->tick += K;
  if (where == VIEKF_HOST) {
    if (int rc = copy_out(s, u, du, bytes, where)) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return VIEKF_OK;
}

int viekf_sim_camera(viekf_sim* s, int32_t num_features, double* z, int32_t* ids, int32_t* count, double* depth, int32_t* landmark,
                     viekf_mem where) {
  if (!s || !z || !ids || !count) return fail(VIEKF_ERR_INVALID, "null argument (z, ids and count are required)");
  if (num_features < 1 || num_features > s->d.MF) return fail(VIEKF_ERR_INVALID, "num_features must be in [1, max_features of viekf_sim_create]");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(s)) return rc;
  const size_t B = s->d.B, N = num_features;
  if (where == VIEKF_DEVICE) {                    // the kernel writes the caller's arrays
    k_sim_camera<<<(unsigned)B, kCamThreads, 0, s->stream>>>(s->d, s->tick, num_features, z, ids, count, depth, landmark);
    HIP_TRY(hipGetLastError());
    return VIEKF_OK;
  }
  // host pointers: one staging block  z | depth | ids | landmark | count
  char* st = nullptr;
  if (int rc = sim_stage(s, 0, 32 * B * N + 4 * B, &st)) return rc;
  double *dz = reinterpret_cast<double*>(st), *dd = reinterpret_cast<double*>(st + 16 * B * N);
  int *di = reinterpret_cast<int*>(st + 24 * B * N), *dl = reinterpret_cast<int*>(st + 28 * B * N), *dc = reinterpret_cast<int*>(st + 32 * B * N);
  k_sim_camera<<<(unsigned)B, kCamThreads, 0, s->stream>>>(s->d, s->tick, num_features, dz, di, dc, depth ? dd : nullptr, landmark ? dl : nullptr);
  HIP_TRY(hipGetLastError());
  int rc;
  if ((rc = copy_out(s, z, dz, 16 * B * N, where)) || (rc = copy_out(s, ids, di, 4 * B * N, where)) ||
      (rc = copy_out(s, count, dc, 4 * B, where)) || (rc = copy_out(s, depth, dd, 8 * B * N, where)) ||
      (rc = copy_out(s, landmark, dl, 4 * B * N, where)))
    return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  return VIEKF_OK;
}

int viekf_sim_render(viekf_sim* s, int32_t width, int32_t height, uint8_t* img, float* depth_mm, viekf_mem where) {
  if (!s || !img) return fail(VIEKF_ERR_INVALID, "null argument");
  if (width < 4 || height < 4 || width > 16384 || height > 16384) return fail(VIEKF_ERR_INVALID, "width and height must be in [4, 16384]");
  if (width & 1) return fail(VIEKF_ERR_INVALID, "width must be even: pixels are stored in pairs (in groups of four when width % 4 == 0)");
  if (int rc = check_where(where)) return rc;
  if (where == VIEKF_DEVICE && ((reinterpret_cast<uintptr_t>(img) & 3) || (reinterpret_cast<uintptr_t>(depth_mm) & 15)))
    return fail(VIEKF_ERR_INVALID, "img must be 4-byte and depth_mm 16-byte aligned");
  if (int rc = set_dev(s)) return rc;
  const size_t npx = (size_t)s->d.B * width * height;
  uint8_t* di = img;
  float* dd = depth_mm;
  if (where == VIEKF_HOST) {
    if (int rc = sim_stage(s, 0, npx, &di)) return rc;
    if (depth_mm)
      if (int rc = sim_stage(s, 1, 4 * npx, &dd)) return rc;
  }
  const int tx = (width + kTileW - 1) / kTileW, ty = (height + kTileH - 1) / kTileH;
  k_sim_render<<<dim3((unsigned)(tx * ty), (unsigned)s->d.B), 256, 0, s->stream>>>(s->d, width, height, tx, di, dd);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    int rc;
    if ((rc = copy_out(s, img, di, npx, where)) || (rc = copy_out(s, depth_mm, dd, 4 * npx, where))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return VIEKF_OK;
}

int viekf_sim_get_truth(viekf_sim* s, double* state, double* t, viekf_mem where) {
  if (!s || (!state && !t)) return fail(VIEKF_ERR_INVALID, "null argument");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(s)) return rc;
  const size_t B = s->d.B;
  double *ds = state, *dt = t;
  if (where == VIEKF_HOST) {
    void* p = nullptr;
    if (int rc = sim_stage(s, 0, 8 * 14 * B, &p)) return rc;
    ds = state ? static_cast<double*>(p) : nullptr;
    dt = t ? static_cast<double*>(p) + 13 * B : nullptr;
  }
  k_sim_get_truth<<<(unsigned)((B + 63) / 64), 64, 0, s->stream>>>(s->d, s->tick, ds, dt);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    int rc;
    if ((rc = copy_out(s, state, ds, 8 * 13 * B, where)) || (rc = copy_out(s, t, dt, 8 * B, where))) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return VIEKF_OK;
}

int viekf_sim_truth_state(viekf_sim* s, const int32_t* ids, int32_t N, double* x_true, viekf_mem where) {
  if (!s || !x_true || (!ids && N > 0)) return fail(VIEKF_ERR_INVALID, "null argument");
  if (N < 0 || N > s->d.MF) return fail(VIEKF_ERR_INVALID, "N must be in [0, max_features of viekf_sim_create]");
  if (int rc = check_where(where)) return rc;
  if (int rc = set_dev(s)) return rc;
  const size_t B = s->d.B, nx = 17 + 5 * (size_t)N;
  const int* dids = ids;
  double* dx = x_true;
  if (where == VIEKF_HOST) {
    void *p0 = nullptr, *p1 = nullptr;
    if (int rc = sim_stage(s, 0, 8 * nx * B, &p0)) return rc;
    if (int rc = sim_stage(s, 1, 4 * B * (N ? N : 1), &p1)) return rc;
    dx = static_cast<double*>(p0);
    if (N > 0) {
      if (int rc = copy_in(s, p1, ids, 4 * B * N, where)) return rc;
      dids = static_cast<const int*>(p1);
    }
  }
  k_sim_truth_state<<<dim3((unsigned)((N + 1 + 63) / 64), (unsigned)B), 64, 0, s->stream>>>(s->d, dids, N, dx);
  HIP_TRY(hipGetLastError());
  if (where == VIEKF_HOST) {
    if (int rc = copy_out(s, x_true, dx, 8 * nx * B, where)) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
  }
  return VIEKF_OK;
}

}  // extern "C"
