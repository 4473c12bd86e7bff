/*
 * viekf_diag.h -- C ABI of the batched consistency diagnostics (libviekf_hip.so): is the error a filter makes the size
 * its covariance says?  NEES, log det P and the innovation statistics (NIS) of every filter of a batch, computed on the
 * device from the lower triangle of P the hot kernels keep current.  The reference has no counterpart (its test ends
 * with "// Check error magnitudes" and no assertion); DESIGN.md §10 has the definitions and the kernels.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch are serialised by the caller.  With VIEKF_DEVICE pointers a call returns once its work
 * is queued; with VIEKF_HOST pointers it returns when the results are in the caller's arrays.
 *
 * Both calls are READ-ONLY: no bit of x, P (the part above the diagonal included), len_features or the status flags
 * changes, nothing is mirrored first (they read the lower triangle of P only), and a participation mask
 * (viekf_batch_set_active) is ignored.  Ring slots selected with viekf_batch_select / viekf_batch_select_filters are
 * followed: filter b is whatever its live (x, P) is.
 */
#ifndef VIEKF_DIAG_H
#define VIEKF_DIAG_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Largest num_features whose factorisation runs entirely in the CU's LDS: the packed lower triangle plus the error row,
 * (n (n + 1) / 2 + n) * 8 bytes with n = 16 + 3 num_features, next to 1 KiB kept for the kernel's static LDS, within
 * 160 KiB (n = 199: 160792 B).  Wider batches take the same algorithm through a device workspace of the batch (at most
 * 256 MiB while one filter's triangle fits that: the batch is processed in chunks of filters). */
#define VIEKF_DIAG_ONCHIP_MAX_FEATURES 61

/* For filter b, with m = 16 + 3 len_features[b], A = P[0:m, 0:m] = L L^T (Cholesky, from the lower triangle):
 *   logdet   [batch]     2 sum_i log L_ii
 *   e                    (x_true [-] x)[0:m]   (viekf_batch_boxminus(x1 = x_true, x2 = the live state))
 *   whitened [batch][n]  y = L^-1 e for i < m, 0 past it
 *   nees     [batch][4]  sum_{i < p} y_i^2 for the leading blocks p = 3 (position), 9 (+ velocity, attitude), 16 (the body
 *                        state), m (everything): the marginal NEES of every leading block, from the one factorisation
 *   info     [batch]     0, or j + 1 for the first pivot j that is not > 0 (a NaN counts).  Then logdet is NaN, whitened is
 *                        NaN from j on, nees[k] is NaN where p_k > j and still reported where p_k <= j; no flag is raised.
 * x_true [batch][nx] may be NULL, then nees and whitened must be NULL too; any output may be NULL, not all of them. */
int viekf_diag_consistency(viekf_batch *b, const double *x_true, double *logdet, double *nees, double *whitened,
                           int32_t *info, viekf_mem where);

/* What VIEKF::update's gate would see (reference vi_ekf_meas.cpp:205-235) at the CURRENT state for each of M measurements
 * of model `type` per filter; nothing is applied between them.  z [batch][M][zdim]; slot [batch][M] for the feature
 * models (QZETA, FEAT, DEPTH, INV_DEPTH), NULL and M == 1 for the others; R rdim x rdim column-major, r_mode 0 one for
 * all, 1 one per filter, 2 one per filter and measurement.
 *   residual [batch][M][3]  q_feat_boxminus (QZETA), the quaternion difference (ATT), z - zhat otherwise; 0 past rdim
 *   S        [batch][M][9]  H P H^T + R, rdim x rdim column-major in the leading entries, 0 after them
 *   nis      [batch][M]     r^T S^-1 r, the number the gate compares with 9
 * A slot that is negative or not an active feature gives NaN in every output of that entry.  residual and S may be NULL.
 * zdim and rdim are taken as given, as viekf_batch_update takes them (1 <= zdim <= 4, 1 <= rdim <= 3; zdim 4 for ATT and
 * QZETA): with other dimensions than the model's the result is the statistic of the leading rdim rows, as the gate of
 * viekf_batch_update would compute it for the same arguments. */
int viekf_diag_innovation(viekf_batch *b, int32_t type, int32_t M, const double *z, int32_t zdim, const int32_t *slot,
                          const double *R, int32_t rdim, int32_t r_mode, double *nis, double *residual, double *S,
                          viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_DIAG_H */
