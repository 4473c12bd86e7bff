/*
 * viekf_sim.h -- C ABI of the batched flight simulator (libviekf_hip.so): `batch` vehicles of vi_ekf_amd/sim.py's
 * Simulator, device-resident, whose outputs are the inputs of the existing entry points: the IMU stream in the layout
 * of viekf_batch_step_n / viekf_batch_propagate_n_to, the feature lists in the layout of viekf_seq_add_frame and
 * viekf_klt_load_image's outputs, GRAY8 frames and depth images in the layout of viekf_klt_load_image /
 * viekf_klt_sample_depth, and the true state in the filter's own layout for viekf_diag_consistency.  The reference has
 * no counterpart (multirotor_sim is an absent submodule and its Monte Carlo driver is stubbed behind MC_SIM);
 * vi_ekf_amd/sim.py is the specification, DESIGN.md §11 has the definitions and the kernels.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback
 * (VIEKF_ERR_NO_DEVICE without a GPU), `where` says whether that call's array pointers are host or device memory (of
 * the simulator's device), and calls on one simulator are serialised by the caller.  With VIEKF_DEVICE pointers a call
 * returns once its work is queued on the simulator's stream; with VIEKF_HOST pointers it returns when the results are
 * in the caller's arrays.  With VIEKF_DEVICE the kernels write the caller's arrays themselves: u must be 16-byte aligned
 * (it is written in 16-byte stores; viekf_sim_imu and viekf_sim_step refuse another pointer), the images as
 * viekf_sim_render says, every other array as its element type.
 *
 * Array layouts (caller-owned, never retained):
 *   u         [K][batch][6] double   raw IMU samples (acc, gyro) in the IMU frame, the `u` of viekf_batch_step_n
 *   z         [batch][num_features][2] double, NaN padding;   ids / landmark [batch][num_features] int32, -1 padding
 *   count     [batch] int32;         depth [batch][num_features] double (m, the range |p_c|), NaN padding
 *   img       [batch][height][width] u8;                      depth_mm [batch][height][width] float (mm, +inf = no hit)
 *   state     [batch][13] double     pos(3) att(4; w x y z) vel_body(3) omega(3), Simulator.state()
 *   x_true    [batch][17 + 5 N] double, the state layout of viekf.h
 *   landmarks [L][3] (shared) or [batch][L][3] double, row i * grid_n + j, L = grid_n^2
 *
 * Noise is counter based: a vehicle's stream depends on (seed, tick, purpose, index) only -- not on the batch, the
 * launch shape or how many ticks one call fuses.  Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 * (tick, stream, block, 0); the four output words w0..w3 give two uniforms in (0, 1),
 *     u1 = ((w0 >> 5) * 2^26 + (w1 >> 6) + 0.5) * 2^-53,      u2 likewise from (w2, w3),
 * and Box-Muller in double gives two normals  sqrt(-2 ln u1) * (cos 2 pi u2, sin 2 pi u2).
 *   stream 0, the IMU at tick k: block 0 -> (acc x, acc y), block 1 -> (acc z, gyr x), block 2 -> (gyr y, gyr z)
 *   stream 1, pixel noise of a frame taken at tick k: block = landmark index -> (x, y)
 * Deliberate difference from sim.py (which draws from one sequential numpy generator): sampling the same tick twice
 * returns the same noise.  sim.py's landmark jitter comes from numpy's PCG64, which is not reproduced: the caller
 * supplies the landmarks.
 */
#ifndef VIEKF_SIM_H
#define VIEKF_SIM_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_SIM_MAX_LANDMARKS 1024

/* what every vehicle of one simulator shares (camera, extrinsics and x0 come from viekf_params) */
typedef struct viekf_sim_config {
  double imu_rate;                      /* Hz; one tick is 1 / imu_rate */
  double accel_sigma, gyro_sigma;       /* white noise of the IMU sample */
  double pix_sigma;                     /* white noise of a reported pixel */
  double grid_origin, grid_pitch;       /* landmark grid: node (i, j) near (origin + i pitch, origin + j pitch, 0) */
  int32_t grid_n;                       /* nodes per side; L = grid_n^2 <= VIEKF_SIM_MAX_LANDMARKS */
  int32_t max_features;                 /* the largest num_features viekf_sim_camera / _truth_state will be given */
  double win_u_min, win_u_max, win_v_min, win_v_max;   /* a landmark is visible strictly inside this pixel window ... */
  double win_min_depth;                 /* ... with p_c.z above this */
} viekf_sim_config;

typedef struct viekf_sim viekf_sim;

/* sim.py's defaults: 250 Hz; sigmas 0.3, 0.01, 0.5; grid -3, 0.22, 28; max_features 12; window 15..625 x 15..465, 0.2 */
int viekf_sim_config_default(viekf_sim_config *c);
/* `batch` vehicles (1 <= batch <= 65535: the vehicle is a grid dimension of the render kernel) at x0, tick 0, nothing
 * tracked; landmarks on the regular grid (no jitter) until set_landmarks;
 * per-vehicle values: seed b + 1, radius 0.35, period 8, accel_bias (0.05, -0.04, 0.03), gyro_bias (0.004, -0.003, 0.002) */
int viekf_sim_create(int32_t batch, const viekf_params *p, const viekf_sim_config *c, int32_t device, viekf_sim **out);
int viekf_sim_destroy(viekf_sim *s);
int viekf_sim_dims(const viekf_sim *s, int32_t *batch, int32_t *landmarks, int32_t *max_features, int64_t *tick);
/* every vehicle back to x0 and tick 0, nothing tracked, next feature id 0; landmarks and per-vehicle values are kept */
int viekf_sim_reset(viekf_sim *s);
/* run later calls on a caller-owned hipStream_t; NULL = HIP's null stream.  A new simulator owns a non-blocking stream. */
int viekf_sim_set_stream(viekf_sim *s, void *hip_stream);
int viekf_sim_sync(viekf_sim *s);
/* per-vehicle values: seed [batch] u64, radius [batch], period [batch] (> 0), accel_bias [batch][3], gyro_bias [batch][3];
 * a NULL array keeps what is set.  Implies viekf_sim_reset.  period > 0 is checked for VIEKF_HOST arrays only: values in
 * device memory are taken as given (a period that is not > 0 gives that vehicle a NaN trajectory). */
int viekf_sim_set_vehicles(viekf_sim *s, const uint64_t *seed, const double *radius, const double *period,
                           const double *accel_bias, const double *gyro_bias, viekf_mem where);
/* the landmark field, shared or one per vehicle; tabulates the blob amplitude 0.55 + 0.45 sin(12.9898 k + 4.1414) of
 * landmark k on the device.  Implies viekf_sim_reset (tracked landmarks are indices into the field).  The simulator holds
 * one field until the first per-vehicle one is set. */
int viekf_sim_set_landmarks(viekf_sim *s, const double *lm, int32_t per_vehicle, viekf_mem where);
/* Simulator.imu() at the current tick, without stepping (sim.imu() before the first run()) */
int viekf_sim_imu(viekf_sim *s, double *u /*[batch][6]*/, viekf_mem where);
/* K IMU periods in one launch, K >= 1: each is _control, _step_truth (four sub-steps), tick += 1, imu() -> u[k] */
int viekf_sim_step(viekf_sim *s, int32_t K, double *u /*[K][batch][6]*/, viekf_mem where);
/* Simulator._camera() with capacity num_features (1 <= num_features <= max_features): tracked landmarks that left the
 * window are dropped and their ids forgotten; the list is refilled from the visible untracked ones, sorted by pixel
 * distance to cam_center (ties by landmark index), taken in the order cand[::3] + cand[1::3] + cand[2::3]; new ids are
 * a running count per vehicle.  A list longer than num_features (the capacity was lowered) is cut to it.
 * z, ids and count are required; depth and landmark may be NULL. */
int viekf_sim_camera(viekf_sim *s, int32_t num_features, double *z, int32_t *ids, int32_t *count, double *depth,
                     int32_t *landmark, viekf_mem where);
/* Simulator.render(): the textured ground plane through the pinhole model, GRAY8, and (depth_mm != NULL) the range in
 * mm as float.  A ray that misses the plane gives grey 30 and +inf.  4 <= width, height <= 16384 and width must be
 * EVEN: the kernel's narrowest store is a pair of pixels (16 bits of grey, 8 bytes of depth); a width that is a
 * multiple of 4 is stored in whole groups of four (32 bits, 16 bytes).  With VIEKF_DEVICE, img must be 4-byte and
 * depth_mm 16-byte aligned.  cam_center and focal_len are those of viekf_params whatever the size. */
int viekf_sim_render(viekf_sim *s, int32_t width, int32_t height, uint8_t *img, float *depth_mm, viekf_mem where);
/* Simulator.state() and the time tick / imu_rate of every vehicle; either may be NULL, not both */
int viekf_sim_get_truth(viekf_sim *s, double *state /*[batch][13]*/, double *t /*[batch]*/, viekf_mem where);
/* The true state in the filter's layout for N feature slots (1 <= N <= max_features; N = 0 with ids NULL gives the body
 * part alone): pos, body-frame vel, att, the vehicle's accel_bias / gyro_bias, mu = x0[16]; slot j whose ids[b][j] is
 * currently tracked holds the bearing quaternion from_two_unit_vectors(e_z, zeta) of zeta = p_c / |p_c| (the rule of
 * VIEKF::init_feature, reference vi_ekf_feat.cpp:6-47, applied to the true bearing) and rho = 1 / |p_c|; a slot whose
 * id is -1 or not tracked holds five NaNs. */
int viekf_sim_truth_state(viekf_sim *s, const int32_t *ids /*[batch][N]*/, int32_t N, double *x_true, viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_SIM_H */
