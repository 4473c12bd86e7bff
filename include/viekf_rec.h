/*
 * viekf_rec.h -- C ABI of the device-resident flight recorder (libviekf_hip.so): the estimated and the true pose of every
 * filter of a batch on every frame of a run, kept in device memory, and the run judged there -- the absolute trajectory error
 * (ATE) after alignment in the directions a visual-inertial filter cannot observe, the relative pose error (RPE) over a frame
 * spacing, the error of the ensemble per frame, and the statistics of up to eight scalar channels (a NEES, say) per frame
 * over the batch and per filter over time.  The reference's own test ends with "// Check error magnitudes" and no assertion
 * (test/vi_ekf_test.cpp:86).  DESIGN.md §15 has the kernels.
 *
 * Conventions are those of viekf.h and viekf_node.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch (and on its companions) are serialised by the caller.  With VIEKF_DEVICE pointers a call
 * returns once its work is queued and nothing synchronises; with VIEKF_HOST pointers it returns when the results are in the
 * caller's arrays.  The recorder uses the batch's size, device and stream ONLY: it never reads or writes x, P, len_features
 * or the status flags, raises no flag and claims no distribution.
 *
 * Definitions.  A pose is {t(3), q(4; w,x,y,z)} in the SE(3) convention viekf.h states with viekf_seq_get_global_pose:
 * T1 * T2 = {t1 + q1.rota(t2), q1 (x) q2}, T^-1 = {-q^-1.rota(t), q^-1}.  q1 [-] q2 is the boxminus of src/quat.cpp:319-327, the
 * one viekf_node_global_error uses; its result is in radians.  The frame index k is ONE counter for the whole recorder, kept
 * on the host (`count`), so that a refusal needs no device round trip.  Per filter b and frame k the recorder holds
 *   est   [7]   the estimated global pose, as viekf_node_global writes it
 *   tru   [7]   {x_true[0:3], x_true[6:10]} of a truth laid out as viekf_sim_truth_state writes it
 *   valid       uint8: (mask == NULL || mask[b] != 0) && all 14 numbers of est and tru are finite -- decided on the device
 *   chan  [K]   `channels` doubles, stored as given; a value that is not finite is left out of every statistic on its own
 * and per frame one double `stamp`, kept on the host.  Poses of a frame that is not valid are stored as given.
 *
 * Every sum below is taken in a fixed order (a lane's own elements ascending, a fixed butterfly inside the wave, the waves in
 * wave order) and without floating-point atomics: two calls on the same recorder agree bit for bit, and so do VIEKF_HOST and
 * VIEKF_DEVICE callers.  A frame range is first <= k < last with 0 <= first <= last <= count; last = -1 means count;
 * T' = last - first.
 */
#ifndef VIEKF_REC_H
#define VIEKF_REC_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_REC_MAX_FRAMES 4096
#define VIEKF_REC_MAX_CHANNELS 8

typedef struct viekf_rec viekf_rec;

/* 1 <= capacity <= VIEKF_REC_MAX_FRAMES frames, 0 <= channels <= VIEKF_REC_MAX_CHANNELS.  b must outlive the recorder. */
int viekf_rec_create(viekf_batch *b, int32_t capacity, int32_t channels, viekf_rec **out);
int viekf_rec_destroy(viekf_rec *rec);
/* count -> 0; what is stored is not cleared, it is out of reach */
int viekf_rec_reset(viekf_rec *rec);
int viekf_rec_count(const viekf_rec *rec, int32_t *count);

/* Appends frame k = count.  est_pose [batch][7]; x_true [batch][ldx], ldx >= 10 (position 0:3, attitude 6:10); chan
 * [batch][channels], which must be NULL exactly when channels == 0; mask [batch] or NULL.  A full recorder
 * (count == capacity) refuses with VIEKF_ERR_INVALID and keeps every bit. */
int viekf_rec_push(viekf_rec *rec, double stamp, const double *est_pose, const double *x_true, int32_t ldx, const double *chan,
                   const uint8_t *mask, viekf_mem where);

/* What is held, T = count: est and tru [batch][T][7], valid [batch][T], chan [T][batch][channels], stamps [T].  NULL skips an
 * array.  Bit for bit what was pushed. */
int viekf_rec_get(viekf_rec *rec, double *est, double *tru, uint8_t *valid, double *chan, double *stamps, viekf_mem where);

/* ATE and RPE of every filter over its valid frames of the range.  With p_e / p_t the estimated / true positions, n their
 * number, c_e / c_t their centroids and A = sum (p_t - c_t)(p_e - c_e)^T (3x3, formed from the centred differences in a pass
 * of its own), the alignment {R_a, t_a} is
 *   align = 0   R_a = I, t_a = 0
 *   align = 1   yaw and translation:  theta = atan2(A10 - A01, A00 + A11) (0 when both arguments are 0), R_a = R_z(theta),
 *               t_a = c_t - R_a c_e
 *   align = 2   SE(3) without scale:  R_a = argmax_R tr(R A^T) by Horn's method -- the eigenvector of the largest eigenvalue
 *               of the symmetric 4x4 matrix built from A, by cyclic Jacobi rotations -- with w >= 0; t_a = c_t - R_a c_e
 *   align_pose [batch][7] = {t_a, q_a}, q_a.rota(v) = R_a v: the aligned estimate is align_pose * T_est
 *   ate_pos    [batch]    = sqrt(mean |p_t - (R_a p_e + t_a)|^2)
 *   ate_att    [batch]    = sqrt(mean |q_t [-] (q_a (x) q_e)|^2)
 * and over the pairs (k, k + delta), both valid and both inside the range, with E = T_k^-1 * T_{k+delta} of the estimate
 * (E_e) and of the truth (E_t) and D = E_t^-1 * E_e
 *   rpe_pos    [batch]    = sqrt(mean |D.t|^2)
 *   rpe_att    [batch]    = sqrt(mean |D.q [-] identity|^2)
 *   n_used     [batch][2] = {n, pairs}
 * n = 0 gives NaN in ate_pos, ate_att and align_pose; pairs = 0 gives NaN in rpe_pos and rpe_att.  delta >= 1.  Each output
 * may be NULL (one at least is needed).  Where the two largest eigenvalues of Horn's matrix coincide (three frames or fewer,
 * collinear positions) R_a is not unique and align_pose is one of the maximisers. */
int viekf_rec_trajectory_error(viekf_rec *rec, int32_t align, int32_t first, int32_t last, int32_t delta, double *ate_pos,
                               double *ate_att, double *rpe_pos, double *rpe_att, double *align_pose, int32_t *n_used,
                               viekf_mem where);

/* Per frame of the range, over the filters valid on it, unaligned and global:
 *   out [T'][4] = {n, sqrt(mean |p_t - p_e|^2), sqrt(mean |q_t [-] q_e|^2), max |p_t - p_e|}
 * n = 0 gives NaN in the three others. */
int viekf_rec_pose_ensemble(viekf_rec *rec, int32_t first, int32_t last, double *out, viekf_mem where);

/* The channels' statistics: per_frame [T'][channels][5] over the batch at one frame, per_filter [batch][channels][5] over the
 * frames of the range, each {n, mean, max, fraction < lo[j], fraction > hi[j]} over the n finite values (the mean of
 * per_frame is the ANEES when the channel holds a NEES; the caller supplies the chi-square bounds).  lo / hi [channels] or
 * NULL: a NULL bound gives fraction 0.  n = 0 gives NaN mean and max and fractions 0.  Either output may be NULL (one is
 * needed).  A recorder without channels refuses. */
int viekf_rec_channels(viekf_rec *rec, int32_t first, int32_t last, const double *lo, const double *hi, double *per_frame,
                       double *per_filter, viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_REC_H */
