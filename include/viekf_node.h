/*
 * viekf_node.h -- C ABI of the device-resident node graph (libviekf_hip.so): the global pose and covariance of every filter
 * of a batch across keyframe resets.  A reset moves the filter's state into a new node frame; what keeps track of where that
 * frame is -- the tail of VIEKF::keyframe_reset (reference src/vi_ekf/vi_ekf_kfr.cpp:147-150), get_global_pose (:14-21),
 * get_global_cov / propagate_global_covariance (:23-53) -- lives here in device memory, fed by the two arrays
 * viekf_frame_intake and viekf_batch_keyframe_reset write (did_reset, edges), so that a closed loop simulator -> step ->
 * intake -> node graph -> diagnostics runs with use_keyframe_reset on and nothing crossing to the host.  The host sequencer
 * (viekf_seq_*) keeps its own node algebra for delayed frames.  DESIGN.md §13 has the kernels.
 *
 * Conventions are those of viekf.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch (and on the node graphs made for it) are serialised by the caller.  With VIEKF_DEVICE
 * pointers a call returns once its work is queued; with VIEKF_HOST pointers it returns when the results are in the
 * caller's arrays.
 *
 * Definitions.  The SE(3) convention is the one viekf.h states with viekf_seq_get_global_pose (T1 * T2, Adj(T), q passive,
 * 6x6 matrices ordered [pos; att] and column-major); it is not restated here.  Per filter, all fp64 except the integers:
 *   node      [7]   {t, q} global pose of the current node frame; identity at start        current_node_global_pose_, vi_ekf.cpp:38
 *   node_cov  [36]  covariance the resets so far have moved out of P; zero at start        global_pose_cov_, vi_ekf.cpp:39
 *   true_node [7]   where the node frame truly is: the reset's map (:120-125) applied to the truth; identity at start
 *   count           int32, the number of resets seen
 *   trail           ring of trail_capacity entries {node before the move [7], edge [17]}: entry count % trail_capacity is
 *                   written by reset number `count` -- what the reference hands its keyframe_reset_callback
 *   edge      [17]  {t(3), q_yaw(4), cov_pos(9, column-major), cov_yaw} as viekf_batch_keyframe_reset reports it
 */
#ifndef VIEKF_NODE_H
#define VIEKF_NODE_H

#include <stdint.h>

#include "viekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_NODE_MAX_TRAIL 4096

typedef struct viekf_node viekf_node;

/* 0 <= trail_capacity <= VIEKF_NODE_MAX_TRAIL (0: no trail is kept).  b must outlive the node graph. */
int viekf_node_create(viekf_batch *b, int32_t trail_capacity, viekf_node **out);
int viekf_node_destroy(viekf_node *nd);
/* identity nodes, zero covariance, count 0, the trail zeroed (pairs with viekf_batch_reset / viekf_frame_reset) */
int viekf_node_reset(viekf_node *nd);

/* The end of keyframe_reset (:147-150) for every filter with did_reset[b] != 0, in this order:
 *   C         = the edge covariance: position block edges[b][7:16] (column-major 3x3), C(5,5) = edges[b][16], zero elsewhere
 *   node_cov += Adj(node)^T C Adj(node)              with the node BEFORE it moves (:149)
 *   trail[count % trail_capacity] = {node, edges[b]} (trail_capacity > 0)
 *   node      = node * {edges[b][0:3], edges[b][3:7]}   (:150)
 *   count    += 1
 *   x_true != NULL:  true_node = {x_true[b][0:3], from_euler(0, 0, yaw(x_true[b][6:10]))} -- the map the reset applies to the
 *                    estimate (:120-125) applied to the truth, evaluated by the very device functions of k_keyframe_reset
 * did_reset [batch], edges [batch][17]: exactly what viekf_frame_intake / viekf_batch_keyframe_reset write.  x_true
 * [batch][ldx], ldx >= 10, the layout of viekf_sim_truth_state (position 0:3, attitude 6:10), or NULL.  A filter with
 * did_reset[b] == 0 keeps every bit.  Values are taken as given: a NaN edge gives a NaN node and no flag is raised. */
int viekf_node_update(viekf_node *nd, const uint8_t *did_reset, const double *edges, const double *x_true, int32_t ldx,
                      viekf_mem where);

/* get_global_pose (:14-21) and get_global_cov (:23-35) of every filter:
 *   pose [batch][7]  = node * {x[POS], x[ATT]}
 *   cov  [batch][36] = node_cov + Adj(node)^T Cx Adj(node),  Cx = the [POS,ATT] x [POS,ATT] blocks of the live P
 * Either may be NULL.  READ-ONLY: x, P, len_features and the status flags keep every bit, and so does the FORM P is stored
 * in -- the 21 elements of P's lower triangle are read where they lie, in the canonical matrix or in the packed image a fused
 * launch left behind, and no conversion of P is launched.  Ring slots selected with viekf_batch_select /
 * viekf_batch_select_filters are followed. */
int viekf_node_global(viekf_node *nd, double *pose, double *cov, viekf_mem where);

/* The truth in the current node frame, which is what the filter estimates: with {t_tn, q_tn} = true_node
 *   x_rel[POS] = q_tn.rotp(x_true[POS] - t_tn),    x_rel[ATT] = q_tn^-1 (x) x_true[ATT],    every other column copied
 * (body-frame velocity, biases, mu and the camera-frame feature states do not depend on the node).  x_true and x_rel
 * [batch][ldx], ldx >= 10; with ldx = nx the result is what viekf_diag_consistency takes as x_true. */
int viekf_node_relative_truth(viekf_node *nd, const double *x_true, double *x_rel, int32_t ldx, viekf_mem where);

/* Global error of the estimate against a truth in the inertial frame, with {pose, cov} of viekf_node_global:
 *   err  [batch][6]  = [x_true[POS] - pose.t ; x_true[ATT] [-] pose.q]      (boxminus of src/quat.cpp:319-327)
 *   nees [batch]     = err^T cov^-1 err through a 6x6 Cholesky factorisation of cov
 *   info [batch]     by the rule of viekf_diag.h: 0, or j + 1 for the first pivot j that is not > 0 (a NaN counts); nees is
 *                    then NaN
 * Each output may be NULL (one at least is needed).  The reference marks its covariance composition as an approximation
 * ("TODO - look at Barfoot's way", :52); this call exists so that it can be measured.  No distribution is claimed. */
int viekf_node_global_error(viekf_node *nd, const double *x_true, int32_t ldx, double *err, double *nees, int32_t *info,
                            viekf_mem where);

/* node [batch][7], node_cov [batch][36], true_node [batch][7], count [batch]: read out / written back, for resuming a run.
 * NULL skips an array. */
int viekf_node_get(viekf_node *nd, double *node, double *node_cov, double *true_node, int32_t *count, viekf_mem where);
int viekf_node_set(viekf_node *nd, const double *node, const double *node_cov, const double *true_node, const int32_t *count,
                   viekf_mem where);

/* The trail as stored: nodes [batch][trail_capacity][7], edges [batch][trail_capacity][17].  Reset number k of a filter is
 * at position k % trail_capacity while count - trail_capacity <= k < count.  Either may be NULL; with trail_capacity 0
 * nothing is written. */
int viekf_node_trail(viekf_node *nd, double *nodes, double *edges, viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_NODE_H */
