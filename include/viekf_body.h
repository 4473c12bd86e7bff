/*
 * viekf_body.h -- C ABI of the fused body-sensor update (libviekf_hip.so): the measurement updates the reference makes
 * outside the camera frame -- ACC and ATT after every propagate in VIEKF_ROS::imu_callback (src/vi_ekf_ros.cpp:172-199),
 * POS, ATT, VEL and ALT in truth_callback (:452-470) -- for every filter of a batch, all of one tick in ONE pass over the
 * covariance.  DESIGN.md §17 has the kernel.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch are serialised by the caller.  With VIEKF_DEVICE pointers a call returns once its work
 * is queued; with VIEKF_HOST pointers it returns when the results are in the caller's arrays.
 */
#ifndef VIEKF_BODY_H
#define VIEKF_BODY_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_BODY_MAX_M 8

/* M body measurements per filter, applied in the caller's order.  1 <= M <= VIEKF_BODY_MAX_M.
 *   types  [M], host      VIEKF_ACC, VIEKF_ALT, VIEKF_ATT, VIEKF_POS or VIEKF_VEL (a model that measures a feature:
 *                         VIEKF_ERR_INVALID)
 *   zdim   [M], host      1 .. 4, what viekf_batch_update takes for the model (ATT: 4, a quaternion; ACC: 2 with the drag
 *                         term, 3 without)
 *   rdim   [M], host      1 .. 3
 *   z      [M][batch][4]  entry m of filter b in the first zdim[m] doubles of its cell; the rest is not read
 *   R      [M][9] (r_mode 0, one per entry) or [M][batch][9] (r_mode 1, one per entry and filter): rdim[m] x rdim[m]
 *                         column-major in the first rdim[m]^2 doubles of the cell
 *   active [M][batch] or NULL (all 1): as viekf_batch_update -- 0 = an inactive measurement, 2 = the filter takes no part
 *                         in this entry
 *   result [M][batch] or NULL: viekf_meas_result per entry and filter
 *   route  host, may be NULL: 1 = the one fused launch, 0 = M launches of viekf_batch_update's kernel
 * z and R must not be NULL (VIEKF_ERR_INVALID).  Nothing is changed by a refused call.
 *
 * The state, the covariance, the result codes and the status bits are what M calls of viekf_batch_update in the same
 * order give (VIEKF::update, src/vi_ekf/vi_ekf_meas.cpp:196-278), on either route.  The fused route works like this, one
 * workgroup per filter:
 *
 * Every body model's H is zero outside the 16 body columns of the error state, so W = P H^T needs only the panel
 * C = P[:, 0:16].  The kernel loads x, lambda, the panel (rows below 16 + 3 len_features[b], from the lower triangle of P
 * only) and D, the diagonal element P(rho, rho) of every feature, into LDS.  Then entry m = 0 .. M-1 runs on them, by the
 * rules and in the order of viekf_batch_update's kernel:
 *   - active == 2: result VIEKF_MEAS_SKIPPED, nothing else.
 *   - a NaN in z: result VIEKF_MEAS_NAN, nothing else.
 *   - active == 0: fix_depth only (src/vi_ekf/vi_ekf_helper.cpp:128-156), result VIEKF_MEAS_SUCCESS.
 *   - otherwise the model and the residual, W_m from the panel's columns in the model's order, S = H W_m + R, its
 *     inverse and the Mahalanobis gate at 9 (:234-239).  Gated: result VIEKF_MEAS_GATED and NO fix_depth.
 *   - the gain K_m = W_m S^-1.  A NaN in K_m or H skips the correction (:247).  Otherwise the state correction (boxplus,
 *     with lambda where use_partial_update is set), the panel update
 *     C[i][c] -= L(i,c) (K_m[max(i,c)] . W_m[min(i,c)]),  L(i,j) = lambda_i + lambda_j - lambda_i lambda_j  (or 1),
 *     and the same downdate on every D[f].  K_m and W_m stay in LDS.
 *   - fix_depth: its two edits of P ( += err^2 where rho < 0,  = P0_feat[2] where rho > 1e2 ) land on D[f]; a later entry
 *     subtracts from the edited value, as it would in memory.  Result VIEKF_MEAS_SUCCESS.
 *   - status bits (VIEKF_FLAG_NAN, VIEKF_FLAG_BLOWUP, VIEKF_FLAG_NEGDEPTH) are ORed after every entry, exactly as M
 *     calls would OR them.
 * One trailing pass over the lower triangle of the active block follows: the panel is stored from C, the rho diagonals
 * from D, and every other element is loaded once, gets  P_ij -= L(i,j) (K_m[i] . W_m[j])  of the entries that were
 * applied, in entry order, and is stored once.  An entry that was skipped, NaN, inactive, gated or guarded contributes
 * nothing.  Rows and columns at or past 16 + 3 len_features[b], the pad rows of a column and everything above the diagonal
 * are neither read nor written; a filter none of whose entries got past the gate is not written at all.  x is written
 * back once.
 *
 * Form of P.  The fused route reads and leaves the LOWER triangle -- the form the fused step hands over and takes back:
 * a packed P is unpacked first, nothing is mirrored, and P counts as current in its lower triangle afterwards (whoever
 * reads it whole, viekf_batch_get_state included, has it mirrored then).  Ring slots selected with viekf_batch_select /
 * viekf_batch_select_filters are followed.
 *
 * Which sizes fuse.  The launch needs viekf_body_lds_bytes(num_features, M) bytes of LDS for its workgroup:
 *   8 (nx' + 18 n + num_features + 6 n M + 64),  nx' = 17 + 5 num_features rounded up to even,  n = 16 + 3 num_features.
 * Where that exceeds viekf_body_lds_limit(device) -- what the device gives one workgroup; at 160 KiB the call fuses up to
 * num_features = 256 for M = 1, 207 for M = 2, 149 for M = 4 and 94 for M = 8 -- the entry point issues the M launches of
 * viekf_batch_update itself, on a P it brings to the full form first, and sets *route = 0.  So would a batch whose P the
 * fused kernel cannot address; every kernel family of this library keeps P as the column-major matrix once it is
 * unpacked, so none is in that case.  The entry point therefore always works. */
int viekf_batch_update_body(viekf_batch *b, int32_t M, const int32_t *types, const int32_t *zdim, const int32_t *rdim,
                            const double *z, const double *R, int32_t r_mode, const uint8_t *active, int32_t *result,
                            int32_t *route, viekf_mem where);

/* Bytes of LDS the fused launch needs for M entries at num_features (0 for arguments out of range); no device needed. */
int64_t viekf_body_lds_bytes(int32_t num_features, int32_t M);
/* Bytes of LDS `device` gives one workgroup. */
int viekf_body_lds_limit(int32_t device, int64_t *bytes);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_BODY_H */
