/*
 * viekf_klt.h -- C ABI of the batched KLT feature tracker (libviekf_hip.so): the reference's image
 * front-end KLT_Tracker (reference src/klt_tracker.cpp:5-170, include/klt_tracker.h) for `batch`
 * cameras at once, device-resident between frames.
 *
 * The tracker is defined by the spec in DESIGN.md §9 (goodFeaturesToTrack + calcOpticalFlowPyrLK at the
 * reference's call sites, OpenCV 3's documented behaviour) with the deviations listed in DESIGN.md §8 and
 * below.  Fixed constants, as the reference hard-codes them: quality 0.3, block size 7, LK window 21x21,
 * at most 3 pyramid levels, 30 iterations, epsilon 0.01, min-eigenvalue threshold 1e-4.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing
 * throws, viekf_last_error() holds the message of the last failing call of this thread, there is no CPU
 * fallback (VIEKF_ERR_NO_DEVICE without a GPU), `where` says whether that call's array pointers are host
 * or device memory (of the tracker's device), and calls on one tracker are serialised by the caller.
 * With VIEKF_DEVICE pointers a call returns once its work is queued on the tracker's stream; with
 * VIEKF_HOST pointers it returns when the results are in the caller's arrays.
 *
 * Array layouts (caller-owned, never retained):
 *   img       [batch][height][width][channels]  u8, channels 1 (GRAY8) or 3 (BGR8)
 *   mask      [height][width] (shared) or [batch][height][width] (per camera), u8: > 1 means "usable"
 *   active    [batch] u8, NULL = every camera; an inactive camera's state is left as it is
 *   features  [batch][max_features][2] double (x, y), clamped to [0, width] x [0, height], NaN padding
 *   ids       [batch][max_features] int32, -1 padding;      count [batch] int32
 *   depth_mm  [batch][height][width] float (mm);            depth [batch][max_features] double (m), NaN padding
 *
 * Kept deviations from the reference:
 *   - the prune's neighbour test is the intended one (distance to the points already kept); the reference
 *     keeps indices into a vector it erases from (klt_tracker.cpp:87-114);
 *   - the replenish mask zeroes the disc dx^2 + dy^2 <= r^2, not OpenCV's rasterised circle;
 *   - drop_features removes the point and its id together (the reference erases from ids_ and from the
 *     post-swap new_features_, not from prev_features_, klt_tracker.cpp:33-47);
 *   - LK samples with float32 bilinear weights, not OpenCV's 14-bit fixed point;
 *   - equal corner scores are ordered by raster position (OpenCV's std::sort leaves ties unspecified);
 *   - sample_depth clamps its read to the image (a saturated coordinate equal to width or height reads out
 *     of bounds in the reference) and, with invert_image, flips the depth image on both axes (the
 *     reference's cv::flip(..., ROTATE_180) passes the flip code 1: a horizontal mirror only).
 */
#ifndef VIEKF_KLT_H
#define VIEKF_KLT_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_KLT_MAX_FEATURES 1024

typedef struct viekf_klt viekf_klt;

/* KLT_Tracker::init (klt_tracker.cpp:10-31) for `batch` cameras: every camera not initialised, next_id 0, mask all 255.
 * 8 <= width, height <= 16384; 1 <= max_features <= VIEKF_KLT_MAX_FEATURES; 0 <= radius <= 1024;
 * invert_image != 0 rotates every input image by 180 degrees (vi_ekf_ros.cpp:269-272). */
int viekf_klt_create(int32_t batch, int32_t width, int32_t height, int32_t max_features, int32_t radius,
                     int32_t invert_image, int32_t device, viekf_klt **out);
int viekf_klt_destroy(viekf_klt *k);
int viekf_klt_dims(const viekf_klt *k, int32_t *batch, int32_t *width, int32_t *height, int32_t *max_features,
                   int32_t *radius, int32_t *levels);
/* every camera back to "not initialised", next_id = 0, no points; the mask is kept */
int viekf_klt_reset(viekf_klt *k);
/* run later calls on a caller-owned hipStream_t; NULL = HIP's null stream.  A new tracker owns a non-blocking stream. */
int viekf_klt_set_stream(viekf_klt *k, void *hip_stream);
int viekf_klt_sync(viekf_klt *k);
/* KLT_Tracker::set_feature_mask (klt_tracker.cpp:49-52): mask = src > 1 ? 255 : 0, shared or one per camera */
int viekf_klt_set_mask(viekf_klt *k, const uint8_t *mask, int32_t per_camera, viekf_mem where);
/* KLT_Tracker::load_image (klt_tracker.cpp:54-170) on every active camera; features / ids / count may be NULL
 * (inactive cameras report the outputs of their last frame) */
int viekf_klt_load_image(viekf_klt *k, const uint8_t *img, int32_t channels, const uint8_t *active, double *features,
                         int32_t *ids, int32_t *count, viekf_mem where);
/* KLT_Tracker::drop_feature (klt_tracker.cpp:33-47) for ids [batch][cnt] (-1 = none); found [batch][cnt] may be NULL.
 * Host pointers. */
int viekf_klt_drop_features(viekf_klt *k, const int32_t *ids, int32_t cnt, uint8_t *found);
/* VIEKF_ROS::color_image_callback's depth read (vi_ekf_ros.cpp:284-297) at the features the last load_image returned:
 * depth_mm[round(y)][round(x)] * 1e-3 as float, NaN if > 1e3 or < min_depth */
int viekf_klt_sample_depth(viekf_klt *k, const float *depth_mm, double min_depth, double *depth, viekf_mem where);
/* the tracked state, unclamped: pts [batch][max_features][2] float, ids [batch][max_features], count [batch], next_id [batch]
 * (any may be NULL).  Host pointers. */
int viekf_klt_get_points(viekf_klt *k, float *pts, int32_t *ids, int32_t *count, int32_t *next_id);
/* pyramid level `level` of the last frame, [batch][h_l][w_l] u8 (h_l, w_l: level 0 is height x width, each next one
 * ((w+1)/2, (h+1)/2)).  Host pointer (tests). */
int viekf_klt_get_level(viekf_klt *k, int32_t level, uint8_t *out);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_KLT_H */
