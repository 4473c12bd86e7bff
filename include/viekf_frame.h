/*
 * viekf_frame.h -- C ABI of the device-resident frame intake (libviekf_hip.so): what VIEKF_ROS::color_image_callback does
 * with a tracked frame (reference src/vi_ekf_ros.cpp:276-305) -- keep_only_features with its keyframe-overlap test, the
 * global id -> local slot lookup of add_measurement(FEAT, id), init_feature for ids the filter has not seen, and the
 * frame's FEAT updates -- for every filter of a batch, with the feature-id bookkeeping in device memory.  This is the
 * ZERO-DELAY route: the frame belongs to the time the filter is at.  Delayed frames, rewind and replay remain the host
 * sequencer's job (viekf_seq_*); composing the keyframe edges into a global node pose is viekf_node.h's.  DESIGN.md §12
 * has the kernels.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch (and on the intakes made for it) are serialised by the caller.  With VIEKF_DEVICE
 * pointers a call returns once its work is queued; with VIEKF_HOST pointers it returns when the results are in the
 * caller's arrays.
 */
#ifndef VIEKF_FRAME_H
#define VIEKF_FRAME_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_FRAME_MAX_M 4096

typedef struct viekf_frame viekf_frame;

/* Device tables for b's batch x num_features: per filter the global ids of its features in slot order (the reference's
 * current_feature_ids_, include/vi_ekf.h) and the keyframe list (keyframe_features_).  b must outlive the intake. */
int viekf_frame_create(viekf_batch *b, viekf_frame **out);
int viekf_frame_destroy(viekf_frame *f);
/* no ids tracked, no keyframe list (pairs with viekf_batch_reset) */
int viekf_frame_reset(viekf_frame *f);
/* Adopts a state written with viekf_batch_set_state: row b of ids [batch][num_features] must hold len_features[b] distinct
 * ids >= 0, then -1.  Host-pointer calls check this and refuse with VIEKF_ERR_INVALID; with device pointers a row's length
 * is the number of its leading ids >= 0.  The keyframe lists are kept. */
int viekf_frame_set_tracked(viekf_frame *f, const int32_t *ids /*[batch][num_features]*/, viekf_mem where);
/* ids [batch][num_features], -1 padded, in slot order -- the layout viekf_sim_truth_state takes; len [batch].  Either may
 * be NULL. */
int viekf_frame_tracked(viekf_frame *f, int32_t *ids, int32_t *len, viekf_mem where);

/* One frame per filter.  1 <= M <= VIEKF_FRAME_MAX_M.
 *   z      [batch][M][2]  pixels, NaN padded           ids [batch][M]  global feature ids, -1 padded
 *   depth  [batch][M] or NULL (NaN): the depth init_feature starts a new feature at
 *   (exactly the shapes viekf_sim_camera, viekf_klt_load_image and viekf_klt_sample_depth write)
 *   R, r_mode             those of viekf_batch_update_feat
 *   active [batch] or NULL (all): 0 = this filter has no frame
 * Outputs, each may be NULL:
 *   result      [batch][M]   viekf_meas_result per entry
 *   gated       [batch][M]   ids of the GATED entries in frame order, -1 padded; gated_count [batch] -- what the callback
 *                            hands to KLT_Tracker::drop_feature
 *   did_reset   [batch]      1 where the overlap test triggered a keyframe reset
 *   edges       [batch][17]  that reset's edge as viekf_batch_keyframe_reset reports it, zeros elsewhere
 *
 * For filter b with active[b] != 0:
 *  1. Entry i with ids[b][i] < 0: VIEKF_MEAS_SKIPPED.  A later entry that repeats an id already seen in this frame:
 *     VIEKF_MEAS_INVALID, and it is ignored from here on.
 *  2. keep_only_features (src/vi_ekf/vi_ekf_feat.cpp:81-117): every tracked id that is not among the frame's ids is removed,
 *     state and covariance compacted exactly as viekf_batch_keep_features does.  An entry with id >= 0 and NaN z still
 *     counts as present.  overlap = the number of kept ids that are in the keyframe list.
 *  3. Keyframe test (:119-139): if use_keyframe_reset, the list is not empty and
 *     (double)overlap / (double)list_size < keyframe_overlap_threshold: a keyframe reset exactly as
 *     viekf_batch_keyframe_reset with this filter in the mask, did_reset[b] = 1, edges[b] filled, list := the frame's ids
 *     (id >= 0, not a repeat, in frame order).  Otherwise, if use_keyframe_reset and the list is empty: list := the
 *     frame's ids.  Otherwise did_reset[b] = 0 and edges[b] is zeros.
 *  4. New features (src/vi_ekf/vi_ekf_meas.cpp:140-146), in frame order: an entry whose z holds no NaN and whose id is not
 *     tracked.  While len < num_features, init_feature(z, depth or NaN) runs and the id is appended to the table.  The
 *     result is VIEKF_MEAS_NEW_FEATURE either way, as the reference answers.
 *  5. Updates: every entry with a tracked id and a z without NaN is one active FEAT update through the batch's own update
 *     path (the kernel family viekf_batch_update_feat would use), in REVERSE frame order -- the order the reference's
 *     queue gives measurements of one stamp (vi_ekf_meas.cpp:150-176).  result is what the update answers (SUCCESS, GATED).
 *     An entry with id >= 0 and a NaN in z: VIEKF_MEAS_NAN (:136-137), tracked or not.
 *  6. gated[b]: the ids of the GATED entries.
 * The new features are initialised BEFORE the updates run (the reference's order within add_measurement calls of one
 * frame; a packed P is then unpacked once per frame).
 * Stale table: if len_features[b] on the device differs from the table's length, somebody edited the features behind the
 * intake's back: filter and table are left untouched bit for bit and every entry with id >= 0 answers
 * VIEKF_MEAS_INVALID (viekf_frame_set_tracked adopts the new state).
 * Inactive filters are untouched: results VIEKF_MEAS_SKIPPED, gated_count 0, did_reset 0.
 * Ring slots selected with viekf_batch_select / viekf_batch_select_filters are followed.  A participation mask
 * (viekf_batch_set_active) in force is refused with VIEKF_ERR_INVALID: the call has its own.
 * The frame's DEPTH measurements (:301-303) are a call of their own behind this one, with this call's ids and result: the
 * intake's depth step, declared in viekf_depth.h beside the update it runs on. */
int viekf_frame_intake(viekf_frame *f, int32_t M, const double *z, const int32_t *ids, const double *depth, const double *R,
                       int32_t r_mode, const uint8_t *active, int32_t *result, int32_t *gated, int32_t *gated_count,
                       uint8_t *did_reset, double *edges, viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_FRAME_H */
