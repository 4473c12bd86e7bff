/*
 * viekf_pixvel.h -- C ABI of the PIXEL_VEL measurement (libviekf_hip.so): the image velocity (optical flow) of tracked
 * features as a measurement, for every filter of a batch.  It is the one model of the reference's table whose h function
 * the authors left empty (h_pixel_vel, src/vi_ekf/vi_ekf_meas.cpp:388-395); viekf_batch_update, viekf_batch_eval_h* and
 * viekf_diag_* keep refusing VIEKF_PIXEL_VEL, and the entry points below are its own.  DESIGN.md section 19 has the model,
 * its derivation and the kernel.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch are serialised by the caller.  With VIEKF_DEVICE pointers a call returns once its work
 * is queued; with VIEKF_HOST pointers it returns when the results are in the caller's arrays.
 *
 * The model.  For the feature in slot i of filter b, with state x and a raw gyro sample g (IMU frame, as u[3:6] of
 * viekf_batch_step_n; rotated by q_b_u exactly as the propagate rotates it):
 *     zhat = Hb(q_zeta) f_zeta(x, g)     [px / s, 2 values]
 * Hb is the 2x2 block h_feat returns (d pixel / d delta, delta the boxplus perturbation of q_zeta) and
 * f_zeta = -T_zeta^T (omega_c + rho zeta x v_c) the bearing's own dynamics at omega = g_b - b_g.  The accelerometer does not
 * enter.  H (2 x n) has nine non-zero columns: VEL (3), B_G (3), the bearing (2) and rho (1).
 * Innovation covariance: S = H P H^T + R + gyro_var J J^T, J the 2x3 B_G block of H (d zhat / d omega = -d zhat / d b_g) and
 * gyro_var >= 0 the variance of one gyro axis of the sample used; the term is part of the effective R of the update.
 * Everything after S is VIEKF::update (vi_ekf_meas.cpp:230-271): gate at 9, K = P H^T S^-1, the NaN guard on K and H, the
 * partial update with lambda or the plain one, boxplus, fix_depth, the status scan.
 */
#ifndef VIEKF_PIXVEL_H
#define VIEKF_PIXVEL_H

#include <stdint.h>

#include "viekf.h"
#include "viekf_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_PIXVELS_MAX_M 256
#define VIEKF_PIXEL_FLOW_MAX_M 4096

/* M PIXEL_VEL measurements per filter.  1 <= M <= VIEKF_PIXVELS_MAX_M.
 *   slot     [batch][M]     feature slot of entry m; a slot may repeat within a call
 *   z        [batch][M][2]  the measured image velocity, px / s (viekf_pixel_flow)
 *   gyro     [batch][3]     the raw gyro sample the measurement is taken at
 *   R        2x2 column-major blocks: one (r_mode 0), [batch] (r_mode 1) or [batch][M] (r_mode 2)
 *   gyro_var >= 0, finite: the variance of one gyro axis
 *   active   [batch][M] or NULL (all 1): as viekf_batch_update -- 0 = an inactive measurement, 2 = the filter takes no part
 *            in this entry
 *   order    0 = entry 0 first; 1 = entry M - 1 first, the order the reference's queue gives the measurements of one stamp
 *   result   [batch][M] or NULL: viekf_meas_result per entry
 *   route    host, may be NULL: 1 = the one fused launch, 0 = M launches of the single-entry kernel
 * slot, z, gyro and R must not be NULL, r_mode is 0 .. 2, order 0 or 1 (VIEKF_ERR_INVALID).  Nothing is changed by a refused
 * call.
 *
 * The entries run in `order`, each by these rules, in this order:
 *   1. active == 2: result VIEKF_MEAS_SKIPPED, nothing else.
 *   2. slot < 0: VIEKF_MEAS_SKIPPED.
 *   3. slot >= len_features[b]: VIEKF_MEAS_INVALID.
 *   4. a component of z or of gyro[b] is NaN: VIEKF_MEAS_NAN, nothing else.
 *   5. active == 0: fix_depth only (src/vi_ekf/vi_ekf_helper.cpp:128-156), result VIEKF_MEAS_SUCCESS, and only fix_depth's
 *      status bits.
 *   6. Otherwise the model and the residual at the current state, W = P H^T from the nine columns, S, and the Mahalanobis gate
 *      at 9.  Gated: VIEKF_MEAS_GATED, NO fix_depth and no status scan.  K = W S^-1; a NaN in K or H skips the correction
 *      (:247).  Otherwise the state correction (boxplus, with lambda where use_partial_update is set) and
 *      P_ij -= L(i, j) (K[max(i, j)] . W[min(i, j)]),  L(i, j) = lambda_i + lambda_j - lambda_i lambda_j (or 1).  Then
 *      fix_depth over all features and the NaN / blow-up scan of x.  Result VIEKF_MEAS_SUCCESS.
 * Status bits (VIEKF_FLAG_NAN, VIEKF_FLAG_BLOWING_UP, VIEKF_FLAG_NEGATIVE_DEPTH) are ORed after every entry.  Every sum runs
 * in a fixed order and nothing but the status word is written with atomics: two runs of one call give bit-equal results.
 *
 * Both routes give the same bits: x, P in the lower triangle of the active block, len, status bits and result codes.  Route 0
 * is the definition.  The fused route (one workgroup per filter) keeps x, lambda, the rho diagonals D (fix_depth's edits land
 * there) and the six body columns VEL, B_G of the current P as an n x 6 panel in LDS; for each entry the feature's three
 * columns are rebuilt left-looking from the start P in memory, which is not written before the end, and the W and S^-1 of the
 * entries applied so far; an applied entry downdates the panel and D; one trailing pass then gives every other element of the
 * lower triangle the applied entries' L(i, j) (K_m[i] . W_m[j]) in entry order: loaded once, stored once.
 *
 * Form of P: the fused route reads and leaves the LOWER triangle (a packed P is unpacked once, nothing is mirrored; whoever
 * reads P whole afterwards has it mirrored then); route 0 reads whole columns, so P is brought to the full form first.
 * Which sizes fuse: the launch needs viekf_pixvels_lds_bytes(num_features, M) bytes of LDS,
 *   8 (nx' + n' + even(N) + 9 n' + 32 + 4 M + 2 n' M),  n' = n rounded up to even
 * -- 150 480 at num_features = M = 50, one workgroup per compute unit.  Where that exceeds viekf_body_lds_limit(device) the
 * entry point runs route 0 itself and says so in *route: it always works.  The M entries are not chunked.
 * Ring slots selected with viekf_batch_select / viekf_batch_select_filters are followed.  A participation mask
 * (viekf_batch_set_active) is NOT consulted, exactly as in viekf_batch_update: a filter that is to sit out gets `active` 2. */
int viekf_batch_update_pixel_vels(viekf_batch *b, int32_t M, const int32_t *slot, const double *z, const double *gyro,
                                  const double *R, int32_t r_mode, double gyro_var, const uint8_t *active, int32_t order,
                                  int32_t *result, int32_t *route, viekf_mem where);

/* Bytes of LDS the fused launch needs for M entries at num_features (0 for arguments out of range); no device needed. */
int64_t viekf_pixvels_lds_bytes(int32_t num_features, int32_t M);

/* Holds this batch's viekf_batch_update_pixel_vels and viekf_frame_intake_pixel_vel to a route: -1 automatic (the default),
 * 0 always the M launches (the definition of the results: tests and measurements compare the fused launch with it), 1 the
 * fused launch where it fits (the same as -1). */
int viekf_batch_pixel_vels_route(viekf_batch *b, int32_t route);

/* Bytes of LDS the single-entry kernel's workgroup needs at num_features (0 for an argument out of range); no device needed:
 *   8 (nx' + 5 n + 32),  nx' = 17 + 5 num_features rounded up to even, n = 16 + 3 num_features
 * -- x, W and K (n x 2 each), lambda and a small scratchpad. */
int64_t viekf_pixvel_lds_bytes(int32_t num_features);

/* Read-only evaluation of the model at the batch's current state, with the device function the update kernel uses (the
 * companion of viekf_batch_eval_h_jacobian, which keeps refusing the type).  The filter is left untouched.
 *   slot  [batch]        feature slot; outside [0, len_features[b]): that filter's zhat and H are NaN
 *   gyro  [batch][3]     raw gyro sample
 *   zhat  [batch][2]
 *   H     [batch][2][n]  dense, row-major per filter, or NULL
 * slot, gyro and zhat must not be NULL. */
int viekf_batch_eval_pixel_vel(viekf_batch *b, const int32_t *slot, const double *gyro, double *zhat, double *H, viekf_mem where);

/* The image velocity of a frame's features from the frame before: a stateless small kernel on the batch's stream.
 * 1 <= M_prev, M <= VIEKF_PIXEL_FLOW_MAX_M.
 *   z_prev [batch][M_prev][2], ids_prev [batch][M_prev]   the earlier frame
 *   z      [batch][M][2],      ids      [batch][M]        the later frame
 *          (the (z, ids) of viekf_sim_camera, viekf_klt_load_image and viekf_frame_intake: NaN / -1 padded)
 *   dt     [batch]  the time between the two frames, s
 *   zdot   [batch][M][2]  (z[b][m] - z_prev[b][k]) / dt[b] where ids_prev[b][k] == ids[b][m] >= 0, all four coordinates are
 *          finite and dt[b] > 0; NaN otherwise.  If ids_prev repeats an id, the first match is used.
 * No argument may be NULL.
 *
 * Such a difference is the MEAN velocity over the interval, that is, to second order, the velocity at its mid-time: a caller
 * who wants the measurement to match the filter's state takes the gyro sample and applies the update near that time, or
 * accepts an error of half a frame interval times the flow's rate of change.  The sequencer (viekf_seq_*) does not queue
 * this type; ordering PIXEL_VEL among other measurements by stamp is the caller's, and out of scope here. */
int viekf_pixel_flow(viekf_batch *b, int32_t M_prev, const double *z_prev, const int32_t *ids_prev, int32_t M, const double *z,
                     const int32_t *ids, const double *dt, double *zdot, viekf_mem where);

/* The pixel-velocity step of the device-resident frame intake, the companion of viekf_frame_intake_depth.  Call it after
 * viekf_frame_intake of the same frame (and after viekf_frame_intake_depth where both are used), with that call's ids and
 * result.  1 <= M <= VIEKF_PIXVELS_MAX_M.
 *   ids           [batch][M]     the frame's ids, as given to viekf_frame_intake
 *   zdot          [batch][M][2]  the flow of each entry (viekf_pixel_flow), NaN where there is none
 *   feat_result   [batch][M]     the `result` viekf_frame_intake wrote for this frame
 *   gyro          [batch][3]     raw gyro sample
 *   R, r_mode                    2x2 column-major blocks: one (0), [batch] (1) or [batch][M] (2)
 *   gyro_var                     as viekf_batch_update_pixel_vels
 *   use_pixel_vel                0 = the measurements are inactive (fix_depth only)
 *   active        [batch] or NULL (all): 0 = this filter has no frame
 *   result        [batch][M] or NULL: viekf_meas_result per entry
 * ids, zdot, feat_result, gyro and R must not be NULL (VIEKF_ERR_INVALID).
 *
 * Entry i of filter b is a measurement where ids[b][i] >= 0, feat_result[b][i] is VIEKF_MEAS_SUCCESS or VIEKF_MEAS_GATED
 * (its FEAT was queued) and both components of zdot[b][i] are finite.  A small kernel finds its slot in the intake's device
 * id table (VIEKF_MEAS_INVALID if the id is no longer there), and the measurements go through
 * viekf_batch_update_pixel_vels' launches with active = use_pixel_vel and order = 1, with no host crossing for device
 * pointers.  Every other entry: VIEKF_MEAS_SKIPPED.  Inactive filters are untouched, all results VIEKF_MEAS_SKIPPED.  Stale
 * table (len_features[b] differs from the table's length): the filter is left bit for bit and every entry with id >= 0
 * answers VIEKF_MEAS_INVALID.  Ring slots are followed; a participation mask in force is refused with VIEKF_ERR_INVALID, as
 * in viekf_frame_intake. */
int viekf_frame_intake_pixel_vel(viekf_frame *f, int32_t M, const int32_t *ids, const double *zdot, const int32_t *feat_result,
                                 const double *gyro, const double *R, int32_t r_mode, double gyro_var, int32_t use_pixel_vel,
                                 const uint8_t *active, int32_t *result, viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_PIXVEL_H */
