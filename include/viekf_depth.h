/*
 * viekf_depth.h -- C ABI of a camera frame's DEPTH updates in one launch (libviekf_hip.so): the DEPTH measurement that
 * VIEKF_ROS::color_image_callback queues behind every FEAT it queued (src/vi_ekf_ros.cpp:287-305), or INV_DEPTH, for
 * every filter of a batch, all of one frame in ONE pass over the covariance, and the frame intake's depth step built on
 * it (viekf_frame_intake_depth, the companion of viekf_frame.h's viekf_frame_intake).  DESIGN.md §18 has the kernel.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch are serialised by the caller.  With VIEKF_DEVICE pointers a call returns once its work
 * is queued; with VIEKF_HOST pointers it returns when the results are in the caller's arrays.
 */
#ifndef VIEKF_DEPTH_H
#define VIEKF_DEPTH_H

#include <stdint.h>

#include "viekf.h"
#include "viekf_body.h"
#include "viekf_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_DEPTHS_MAX_M 256

/* M measurements of ONE model per filter.  1 <= M <= VIEKF_DEPTHS_MAX_M.
 *   type   VIEKF_DEPTH or VIEKF_INV_DEPTH (anything else: VIEKF_ERR_INVALID)
 *   slot   [batch][M]  feature slot of entry m; a slot may repeat within a call
 *   z      [batch][M]  the measured depth (DEPTH) or inverse depth (INV_DEPTH)
 *          (the shapes viekf_sim_camera, viekf_klt_sample_depth and viekf_frame_intake use)
 *   R      one double (r_mode 0), [batch] (r_mode 1) or [batch][M] (r_mode 2): the variance
 *   active [batch][M] or NULL (all 1): as viekf_batch_update -- 0 = an inactive measurement, 2 = the filter takes no part
 *          in this entry
 *   order  0 = entry 0 first; 1 = entry M - 1 first, the order the reference's queue gives the measurements of one stamp
 *          (src/vi_ekf/vi_ekf_meas.cpp:150-176), which viekf_frame_intake uses for FEAT
 *   result [batch][M] or NULL: viekf_meas_result per entry
 *   route  host, may be NULL: 1 = the one fused launch, 0 = M launches of viekf_batch_update's kernel
 * slot, z and R must not be NULL, r_mode is 0 .. 2, order 0 or 1 (VIEKF_ERR_INVALID).  Nothing is changed by a refused call.
 *
 * The state, the covariance, the result codes and the status bits are what M calls of viekf_batch_update(type, ...) in
 * that order give (VIEKF::update, src/vi_ekf/vi_ekf_meas.cpp:196-278), on either route.  The fused route works like this,
 * one workgroup per filter:
 *
 * h_depth has one non-zero element of H, H(0, c) = -1 / rho^2 at c = 16 + 3 slot + 2, h_inv_depth H(0, c) = 1 at the
 * same column (:369-386).  So W_m = P H^T is one column of the current P times a scalar, S is a scalar and
 * K_m = W_m / S.  The kernel loads x, lambda, D = the diagonal element P(rho, rho) of every feature, and for every entry
 * the column c of the P it starts from (from the lower triangle only: P[i + c ld] for i >= c, P[c + i ld] above) into
 * LDS.  Then the entries run in `order`, each by the rules and in the order of viekf_batch_update's kernel:
 *   1. active == 2: result VIEKF_MEAS_SKIPPED, nothing else.
 *   2. slot < 0: VIEKF_MEAS_SKIPPED.
 *   3. slot >= len_features[b]: VIEKF_MEAS_INVALID.
 *   4. z is NaN: VIEKF_MEAS_NAN, nothing else.
 *   5. active == 0: fix_depth only (src/vi_ekf/vi_ekf_helper.cpp:128-156), result VIEKF_MEAS_SUCCESS, and only
 *      fix_depth's status bits.
 *   6. Otherwise the model and the residual at the current state; the column of the CURRENT P, left-looking:
 *        P_now(i, c) = P_0(i, c) - sum over the entries k applied so far, in order, of
 *                      L(i, c) (K_k[max(i, c)] W_k[min(i, c)]),  L(i, j) = lambda_i + lambda_j - lambda_i lambda_j (or 1
 *      without use_partial_update), with P_now(c, c) taken from D; W_m = that column times H; S = H W_m[c] + R, and the
 *      Mahalanobis gate at 9 (:234-239).  Gated: result VIEKF_MEAS_GATED, NO fix_depth and no status scan.
 *      The gain K_m = W_m S^-1.  A NaN in K_m or H skips the correction (:247).  Otherwise the state correction runs on
 *      all of x (boxplus, with lambda where use_partial_update is set), every D[f] takes the entry's downdate, and W_m and
 *      S^-1 stay in LDS for the entries after it.  Then fix_depth runs over all features -- its two edits of P
 *      ( += err^2 where rho < 0,  = P0_feat[2] where rho > 1e2 ) land on D[f], and a later entry subtracts from the edited
 *      value, as it would in memory -- then the NaN / blow-up scan of x.  Result VIEKF_MEAS_SUCCESS.
 *   Status bits (VIEKF_FLAG_NAN, VIEKF_FLAG_BLOWING_UP, VIEKF_FLAG_NEGATIVE_DEPTH) are ORed after every entry, exactly as
 *   M calls would OR them.
 * One trailing pass over the lower triangle of the active block follows: the rho diagonals are stored from D, and every
 * other element is loaded once, gets  P_ij -= L(i, j) (K_m[i] W_m[j])  of the applied entries, in entry order, and is
 * stored once.  An entry that was skipped, invalid, NaN, inactive, gated or guarded contributes nothing.  Every sum runs
 * in a fixed order and nothing is accumulated with atomics: two runs of one call give bit-equal results.
 *
 * What is not touched: rows and columns at or past 16 + 3 len_features[b], the pad rows of a column and everything
 * above the diagonal are neither read nor written.  A filter none of whose entries was applied gets no write to P beyond
 * the rho diagonals that fix_depth edited; a filter all of whose entries answer SKIPPED, INVALID, NAN or GATED is left bit
 * for bit, x included.
 *
 * Form of P.  The fused route reads and leaves the LOWER triangle, as viekf_batch_update_body does: a packed P is
 * unpacked once, nothing is mirrored, and P counts as current in its lower triangle afterwards (whoever reads it whole,
 * viekf_batch_get_state included, has it mirrored then).  Ring slots selected with viekf_batch_select /
 * viekf_batch_select_filters are followed.  A participation mask (viekf_batch_set_active) is NOT consulted, exactly as in
 * viekf_batch_update and viekf_batch_update_body: a filter that is to sit out gets `active` 2 in its row.
 *
 * Which sizes fuse.  The launch needs viekf_depths_lds_bytes(num_features, M) bytes of LDS for its workgroup:
 *   8 (even(nx' + n + num_features) + 2 + even(M) + n' M),  nx' = 17 + 5 num_features rounded up to even,
 *   n = 16 + 3 num_features, n' = n rounded up to even, even(v) = v rounded up to even
 * -- x, lambda, D, a guard word, S^-1 per entry, and one row of n' doubles per entry that holds first the entry's start
 * column and then an applied entry's W.  That is 70 688 bytes at num_features = M = 50 (two workgroups per compute unit)
 * and 159 216 at 77.
 * Where it exceeds viekf_body_lds_limit(device) -- what the device gives one workgroup; at 160 KiB num_features = M fuses
 * up to 78, M = 256 up to num_features = 20 -- the entry point issues the M launches of viekf_batch_update's kernel itself,
 * on a P it brings to the full form first, gathering entry m of every filter with a small kernel (no host copy for device
 * pointers), and sets *route = 0.  The entry point therefore always works. */
int viekf_batch_update_depths(viekf_batch *b, int32_t type, int32_t M, const int32_t *slot, const double *z, const double *R,
                              int32_t r_mode, const uint8_t *active, int32_t order, int32_t *result, int32_t *route,
                              viekf_mem where);

/* Bytes of LDS the fused launch needs for M entries at num_features (0 for arguments out of range); no device needed. */
int64_t viekf_depths_lds_bytes(int32_t num_features, int32_t M);

/* The depth step of the device-resident frame intake: the DEPTH measurements of a frame (src/vi_ekf_ros.cpp:301-303).  Call it
 * after viekf_frame_intake of the same frame, with that call's ids and result.  1 <= M <= VIEKF_DEPTHS_MAX_M.
 *   ids         [batch][M]  the frame's ids, as given to viekf_frame_intake
 *   depth       [batch][M]  the depth at each entry's pixel (viekf_klt_sample_depth, viekf_sim_camera), NaN where there is none
 *   feat_result [batch][M]  the `result` viekf_frame_intake wrote for this frame
 *   R, r_mode               the DEPTH variance: one double (0), [batch] (1) or [batch][M] (2)
 *   use_depth               0 = the measurements are inactive (the reference's use_depth_ false: fix_depth only, :230)
 *   active      [batch] or NULL (all): 0 = this filter has no frame
 *   result      [batch][M] or NULL: viekf_meas_result per entry
 * ids, depth, feat_result and R must not be NULL (VIEKF_ERR_INVALID).
 *
 * Entry i of filter b is a DEPTH measurement where ids[b][i] >= 0, feat_result[b][i] is VIEKF_MEAS_SUCCESS or
 * VIEKF_MEAS_GATED -- where the reference's add_measurement(FEAT) answered MEAS_SUCCESS when it queued the entry: a new
 * feature, a NaN pixel or a repeated id gets no DEPTH -- and depth[b][i] is finite.  A small kernel finds its slot in the
 * intake's device id table (VIEKF_MEAS_INVALID if the id is no longer there), and the measurements go through
 * viekf_batch_update_depths with active = use_depth and order = 1 (reverse frame order, as the frame's FEAT updates), with
 * no host crossing for device pointers.  Every other entry: VIEKF_MEAS_SKIPPED.
 * Inactive filters are untouched, all results VIEKF_MEAS_SKIPPED.  Stale table (len_features[b] differs from the table's
 * length): the filter is left bit for bit and every entry with id >= 0 answers VIEKF_MEAS_INVALID.  Ring slots are
 * followed; a participation mask in force is refused with VIEKF_ERR_INVALID, as in viekf_frame_intake.
 *
 * Kept deviation.  The reference's queue alternates a frame's DEPTH(i) and FEAT(i).  Here the frame's FEAT updates run
 * first (viekf_frame_intake) and its DEPTH updates after them, as vi_ekf_amd/klt.py::track_frame already groups them. */
int viekf_frame_intake_depth(viekf_frame *f, int32_t M, const int32_t *ids, const double *depth, const int32_t *feat_result,
                             const double *R, int32_t r_mode, int32_t use_depth, const uint8_t *active, int32_t *result,
                             viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_DEPTH_H */
