/*
 * viekf_cam.h -- C ABI of the device-resident camera model (libviekf_hip.so): radial-tangential lens distortion
 * (k1, k2, p1, p2, the four-element `distortion:` key of the reference's params/ocam.yaml, leo.yaml, firefly.yaml and
 * ekf.yaml, which nothing in the reference's src/ reads) for `batch` cameras at once.  Every stage after the tracker --
 * h_feat, init_feature, the simulator's render -- assumes an ideal pinhole; the tracker reports pixels of the RAW image.
 * This handle goes between the two: points and their measurement noise from raw to ideal pixels, the mask that keeps a
 * tracker inside the model, and whole images warped either way.  DESIGN.md §16 has the definitions and the kernels;
 * tests/cam_ref.py restates every operation below in numpy.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback
 * (VIEKF_ERR_NO_DEVICE without a GPU), `where` says whether that call's array pointers are host or device memory (of
 * the camera's device), and calls on one camera model are serialised by the caller.  With VIEKF_DEVICE pointers a call
 * returns once its work is queued on the handle's stream; with VIEKF_HOST pointers it returns when the results are in
 * the caller's arrays.  With VIEKF_DEVICE the kernels read and write the caller's arrays themselves: doubles 8-byte,
 * int32 4-byte aligned, images as viekf_cam_warp says.
 *
 * The model, operation by operation (double throughout, no fused multiply-add).  One intrinsics set holds the raw
 * camera (f, c, k1 k2 p1 p2), the pinhole the filter uses (F, C = out_focal, out_center), min_det and the derived r_valid.
 *
 *   forward(x, y):   r2  = x x + y y
 *                    rad = 1 + k1 r2 + k2 r2 r2               drad = k1 + 2 k2 r2
 *                    xd  = x rad + 2 p1 x y + p2 (r2 + 2 x x)
 *                    yd  = y rad + p1 (r2 + 2 y y) + 2 p2 x y
 *                    J00 = rad + 2 x x drad + 2 p1 y + 6 p2 x
 *                    J01 = J10 = 2 x y drad + 2 p1 x + 2 p2 y
 *                    J11 = rad + 2 y y drad + 6 p1 y + 2 p2 x
 *                    det = J00 J11 - J01 J10
 *   inside(x, y):    r2 <= r_valid^2  and  det > min_det
 *
 *   distort (ideal pixel (u, v) -> raw pixel):   x = (u - C0) / F0, y = (v - C1) / F1, forward,
 *                    raw = (f0 xd + c0, f1 yd + c1),  J = d raw / d ideal = [f0 J00 / F0, f1 J10 / F0, f0 J01 / F1, f1 J11 / F1]
 *                    (column-major).  No validity test: a point beyond the fold is mapped as the polynomial says.
 *
 *   undistort (raw pixel (u, v) -> ideal pixel):  xd = (u - c0) / f0, yd = (v - c1) / f1;  (x, y) = (xd, yd);
 *                    at most VIEKF_CAM_MAX_ITER times:  forward(x, y); not inside -> OUT_OF_MODEL;
 *                        ex = xd - xd(x, y), ey = yd - yd(x, y);
 *                        sx = (J11 ex - J01 ey) / det, sy = (J00 ey - J10 ex) / det;  x += sx, y += sy;
 *                        stop when sx sx + sy sy <= VIEKF_CAM_STEP_TOL^2
 *                    no stop within VIEKF_CAM_MAX_ITER -> OUT_OF_MODEL;  forward(x, y) once more at the solution,
 *                    not inside -> OUT_OF_MODEL;  ideal = (F0 x + C0, F1 y + C1);
 *                    J_u = d ideal / d raw = [[F0 J11 / det / f0, -F0 J01 / det / f1], [-F1 J10 / det / f0, F1 J00 / det / f1]];
 *                    R_out = J_u R J_u^T with T = J_u R first, then R_out00, R_out10, R_out11 from T and J_u, R_out01 = R_out10.
 *
 * A bare "det > 0 along the iteration" test is not enough: Newton can jump the fold of a barrel lens into the outer region
 * where det is positive again and return a wrong preimage.  So the host derives r_valid for every set: on the polar scan
 * r = i * VIEKF_CAM_SCAN_STEP (i = 1 ..), r <= VIEKF_CAM_SCAN_CAP, directions 2 pi j / VIEKF_CAM_SCAN_DIRS, r_valid is the
 * largest scanned radius such that every sample at a smaller or equal radius has det > min_det (0 when the first ring
 * fails).  Every iterate, the start (xd, yd) included, must be inside: a raw point whose own normalised radius exceeds
 * r_valid is outside the model whatever its preimage (this matters for a pincushion lens only, whose det never falls and
 * whose r_valid is the cap).
 *
 * Array layouts (caller-owned, never retained):
 *   z_ideal, z_raw  [batch][M][2] double, NaN padding;    J, R_out [batch][M][4] double, column-major 2 x 2
 *   R               [4], [batch][4] or [batch][M][4] double by r_mode 0, 1, 2, column-major, as viekf_batch_update_feat takes it
 *   status          [batch][M] int32
 *   mask            [height][width] (one shared set) or [batch][height][width] u8, as viekf_klt_set_mask takes it
 *   src, dst        [batch][height][width] u8;            src_depth, dst_depth [batch][height][width] float (mm, +inf = none)
 */
#ifndef VIEKF_CAM_H
#define VIEKF_CAM_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_CAM_MAX_ITER 20
#define VIEKF_CAM_STEP_TOL 1e-14          /* normalised units; the stop is |step|^2 <= tol^2 */
#define VIEKF_CAM_SCAN_STEP 0.00390625    /* 2^-8 */
#define VIEKF_CAM_SCAN_CAP 4.0            /* 1024 rings: 76 degrees off the axis, past any lens this model fits */
#define VIEKF_CAM_SCAN_DIRS 32
#define VIEKF_CAM_MAX_M 4096

/* status of one undistorted point */
#define VIEKF_CAM_OK 0
#define VIEKF_CAM_PADDING 1               /* a NaN in z_raw: NaN out, R_out = the entry's input R */
#define VIEKF_CAM_OUT_OF_MODEL 2          /* NaN out, R_out = the entry's input R */

/* direction of viekf_cam_warp */
#define VIEKF_CAM_RECTIFY 0               /* src raw -> dst ideal */
#define VIEKF_CAM_DISTORT 1               /* src ideal -> dst raw */

typedef struct viekf_cam_intrinsics {
  double focal[2], center[2];             /* of the RAW image */
  double dist[4];                         /* k1 k2 p1 p2, the order of the YAML key */
  double out_focal[2], out_center[2];     /* the pinhole the filter uses: viekf_params.focal_len / cam_center */
  double min_det;                         /* a point is inside the model where det J_d > min_det; default 0 */
} viekf_cam_intrinsics;

typedef struct viekf_cam viekf_cam;

/* focal 1, 1; centre 0, 0; no distortion; out_* the same; min_det 0 */
int viekf_cam_intrinsics_default(viekf_cam_intrinsics *k);
/* cam_center, focal_len and distortion (absent: zeros) of the parameter file `path`; out_focal / out_center are the
 * focal_len / cam_center of `params_path`, or of `path` itself when params_path is NULL; min_det 0 */
int viekf_cam_load_yaml(const char *path, const char *params_path, viekf_cam_intrinsics *out);

/* `batch` cameras (1 <= batch <= 65535: the camera is a grid dimension of the pixel kernels), all with the default set */
int viekf_cam_create(int32_t batch, int32_t device, viekf_cam **out);
int viekf_cam_destroy(viekf_cam *c);
/* sets = 1 while one set is shared, batch after a per-camera call */
int viekf_cam_dims(const viekf_cam *c, int32_t *batch, int32_t *sets);
/* run later calls on a caller-owned hipStream_t; NULL = HIP's null stream.  A new handle owns a non-blocking stream. */
int viekf_cam_set_stream(viekf_cam *c, void *hip_stream);
int viekf_cam_sync(viekf_cam *c);
/* one set for every camera (per_camera = 0) or k[batch].  HOST memory only -- the host derives r_valid per set -- and
 * a pointer into device memory is refused.  focal and out_focal must be > 0 and every field finite.  Waits for the
 * handle's stream before the table changes. */
int viekf_cam_set_intrinsics(viekf_cam *c, const viekf_cam_intrinsics *k, int32_t per_camera);
/* the sets as they stand, k[sets] and r_valid[sets] (either may be NULL); host memory */
int viekf_cam_get_intrinsics(const viekf_cam *c, viekf_cam_intrinsics *k, double *r_valid);

/* the forward model in closed form, 1 <= M <= VIEKF_CAM_MAX_M; J may be NULL */
int viekf_cam_distort_points(viekf_cam *c, int32_t M, const double *z_ideal, double *z_raw, double *J, viekf_mem where);
/* the inverse model with the measurement noise; R_out (always the r_mode 2 layout viekf_frame_intake takes) and status
 * may be NULL; R may be NULL when R_out is */
int viekf_cam_undistort_points(viekf_cam *c, int32_t M, const double *z_raw, const double *R, int32_t r_mode,
                               double *z_ideal, double *R_out, int32_t *status, viekf_mem where);
/* 255 where undistorting the raw pixel centre (x, y) gives VIEKF_CAM_OK, 0 elsewhere; [height][width] while one set is
 * shared, [batch][height][width] otherwise.  Sizes and alignment as viekf_cam_warp's dst. */
int viekf_cam_valid_mask(viekf_cam *c, int32_t width, int32_t height, uint8_t *mask, viekf_mem where);
/* VIEKF_CAM_RECTIFY: output pixel (u, v) of the ideal image is distorted and src (raw) sampled there; the pixel is
 * outside the model when its (x, y) is not inside.  VIEKF_CAM_DISTORT: output pixel (u, v) of the raw image is
 * undistorted and src (ideal, e.g. viekf_sim_render's) sampled there; outside the model when the status is not OK.
 * Sampling at (sx, sy): outside [0, width - 1] x [0, height - 1] (or NaN) -> `fill` and +inf depth, as for a pixel outside
 * the model.  Grey: x0 = floor(sx), x1 = min(x0 + 1, width - 1), ax = sx - x0, likewise y;
 * v = (1 - ay) ((1 - ax) I[y0][x0] + ax I[y0][x1]) + ay ((1 - ax) I[y1][x0] + ax I[y1][x1]) in double, floor(v + 0.5).
 * Depth: src_depth[floor(sy + 0.5)][floor(sx + 0.5)], never blended.  src_depth and dst_depth are given together or not
 * at all.  4 <= width, height <= 16384 and width must be EVEN (pixels are stored in pairs, in groups of four when width
 * is a multiple of 4), as viekf_sim_render; with VIEKF_DEVICE dst must be 4-byte and dst_depth 16-byte aligned.  src and
 * dst must not overlap. */
int viekf_cam_warp(viekf_cam *c, int32_t direction, int32_t width, int32_t height, const uint8_t *src, uint8_t *dst,
                   const float *src_depth, float *dst_depth, int32_t fill, viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_CAM_H */
