/*
 * viekf_map.h -- C ABI of the device-resident landmark map (libviekf_hip.so): what every filter of a batch believes about
 * the world.  A feature is held as a bearing quaternion q_zeta and an inverse depth rho in the camera frame of the current
 * node; here it becomes a 3-D position in metres with a 3x3 covariance, in the node frame and in the global frame, live
 * (viekf_map_landmarks), kept across feature loss and keyframe resets in a store keyed by the frame intake's feature ids
 * (viekf_map_update, _get, _set), and held against the landmark the simulator drew it from (viekf_map_error).  The reference
 * gets as far as a commented-out overlay of estimated against measured features (src/vi_ekf_ros.cpp:316-323).  DESIGN.md §14
 * has the kernels.
 *
 * Conventions are those of viekf.h and viekf_node.h: every call returns VIEKF_OK or a negative viekf_status, nothing throws,
 * viekf_last_error() holds the message of the last failing call of this thread, there is no CPU fallback, `where` says
 * whether that call's array pointers are host or device memory (of the batch's device), the work runs on the batch's
 * stream, and calls on one batch (and on its companions) are serialised by the caller.  With VIEKF_DEVICE pointers a call
 * returns once its work is queued and nothing synchronises; with VIEKF_HOST pointers it returns when the results are in the
 * caller's arrays.  Ring slots selected with viekf_batch_select / viekf_batch_select_filters are followed.  Every call is
 * READ-ONLY on the batch -- x, the lower triangle of P, len_features and the status flags keep every bit -- and therefore
 * ignores a participation mask (viekf_batch_set_active).  A P that a fused launch left packed is brought to the canonical
 * lower form first, exactly as viekf_diag_consistency does; it is never mirrored.
 *
 * Geometry.  R(q) is passive, rota(q, v) = R(q)^T v, rotp(q, v) = R(q) v, x = [pos, vel, att, b_a, b_g, mu, (q_zeta, rho)...],
 * the error state has dxPOS at 0..2, dxATT at 6..8 and feature j at 16+3j..18+3j (viekf.h).  For slot j < len_features:
 *   zeta  = rota(q_zeta, e_z),  p_c = zeta / rho,  b = p_b_c + rota(q_b_c, p_c)
 *   l     = pos + rota(att, b)                                      the landmark in the node frame
 *   l_G   = node.t + rota(node.q, l)                                T1 * T2 of viekf.h applied to a point; node is the node
 *                                                                   graph's current node, the identity without a node graph
 *   Sigma = J P9 J^T                                                P9: rows and columns {0,1,2, 6,7,8, 16+3j,17+3j,18+3j}
 *                                                                   of the live P (45 elements of the lower triangle)
 *   J (3x9) = d l(x [+] d) / d d at d = 0 for the filter's own boxplus (vi_ekf_helper.cpp:88-98):
 *     d l / d pos  = I                                              d l / d att = -R(att)^T [b]x
 *     d l / d zeta = -R(att)^T R(q_b_c)^T [zeta]x T_zeta / rho      d l / d rho = -R(att)^T R(q_b_c)^T zeta / rho^2
 *   Sigma_G = R(node.q)^T Sigma R(node.q)
 * The node's own covariance (node_cov of viekf_node.h) is NOT folded into Sigma_G: the reference marks its composition as an
 * approximation ("TODO - look at Barfoot's way", vi_ekf_kfr.cpp:52), and viekf_node_global already hands it out.
 * A slot at or past len_features, or one whose rho is not finite or not > 0, gives NaN in every output of that slot and does
 * not enter the store; no status flag is raised.  Covariances are 6 doubles, the lower triangle in the order
 * xx, yx, yy, zx, zy, zz.
 */
#ifndef VIEKF_MAP_H
#define VIEKF_MAP_H

#include <stdint.h>

#include "viekf.h"
#include "viekf_frame.h"
#include "viekf_node.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIEKF_MAP_MAX_CAPACITY 4096

typedef struct viekf_map viekf_map;

/* 0 <= capacity <= VIEKF_MAP_MAX_CAPACITY entries of the store per filter (0: no store, the live query only).  frame: the
 * batch's frame intake or NULL; capacity > 0 and viekf_map_error need it (the store is keyed by the intake's id table).
 * node: the batch's node graph or NULL (then every node is the identity and node_count 0).  frame and node must have been
 * made for b; b, frame and node must outlive the map. */
int viekf_map_create(viekf_batch *b, viekf_frame *frame, viekf_node *node, int32_t capacity, viekf_map **out);
int viekf_map_destroy(viekf_map *m);
/* every entry of the store empty: id -1, everything else zero (pairs with viekf_batch_reset / viekf_frame_reset) */
int viekf_map_reset(viekf_map *m);

/* The live query: pos_node / pos_global [batch][num_features][3] = l / l_G, cov_node / cov_global [batch][num_features][6] =
 * Sigma / Sigma_G of every slot.  Each may be NULL (one at least is needed). */
int viekf_map_landmarks(viekf_map *m, double *pos_node, double *cov_node, double *pos_global, double *cov_global,
                        viekf_mem where);

/* Every valid tracked slot into the store.  The store holds `capacity` entries per filter, each
 *   {id (-1: empty), pos_G [3], cov_G [6], n_obs, node_count}
 * and the feature with the intake's id g goes to entry g % capacity: {g, l_G, Sigma_G, n_obs, node_count} with n_obs = the
 * entry's n_obs + 1 when the entry held g already and 1 otherwise, node_count = the node graph's reset count now.  When two
 * tracked ids of one filter share a residue in one call the LARGER id is written and the other is not (decided by comparing
 * ids inside the launch, never by store order).  Entries of features that are no longer tracked keep every bit: this is how
 * the map survives feature loss and resets.  A filter whose id table is stale (len_features differs from the table's length,
 * the rule of viekf_frame_intake) keeps its store untouched.  With capacity 0 the call does nothing.
 * CALL IT AFTER viekf_node_update OF THE SAME FRAME: l_G is composed with the node as it is now, and between a frame's reset
 * and the node's move the state is already in the new node frame while the node is still the old one.  This cannot be
 * checked here. */
int viekf_map_update(viekf_map *m);

/* The store as held, for reading out a point cloud and for resuming a run bit for bit: ids [batch][capacity],
 * pos [batch][capacity][3], cov [batch][capacity][6], n_obs [batch][capacity], node_count [batch][capacity].  NULL skips an
 * array. */
int viekf_map_get(viekf_map *m, int32_t *ids, double *pos, double *cov, int32_t *n_obs, int32_t *node_count, viekf_mem where);
int viekf_map_set(viekf_map *m, const int32_t *ids, const double *pos, const double *cov, const int32_t *n_obs,
                  const int32_t *node_count, viekf_mem where);

/* The metric landmark error of every slot.  lm_true [L][3] (per_vehicle == 0) or [batch][L][3]: the landmark field.
 * frame_ids and landmark [batch][M], 1 <= M <= VIEKF_FRAME_MAX_M, exactly as viekf_sim_camera writes ids and landmark: the
 * intake's id of slot j is looked up in frame_ids[b] (the first match, the lookup of viekf_sim_truth_state), the entry's
 * landmark k gives l_true = lm_true[k].
 *   err_node   [batch][num_features][3] = rotp(true_node.q, l_true - true_node.t) - l    (true_node of viekf_node.h; the
 *                                                                                         identity without a node graph)
 *   nees       [batch][num_features]    = err_node^T Sigma^-1 err_node through a 3x3 Cholesky factorisation
 *   info       [batch][num_features]    by the rule of viekf_diag.h: 0, or p + 1 for the first pivot p that is not > 0 (a
 *                                         NaN counts); nees is then NaN
 *   err_global [batch][num_features][3] = l_true - l_G.  It has no NEES: the node's uncertainty is not in Sigma_G.
 * A slot that gives NaN in viekf_map_landmarks, one whose id is not in the frame or whose landmark is < 0 or >= L, and every
 * slot of a filter whose id table is stale gives NaN and info 0.  Each output may be NULL (one at least is needed).  Needs
 * the frame intake. */
int viekf_map_error(viekf_map *m, const double *lm_true, int32_t per_vehicle, int32_t L, const int32_t *frame_ids,
                    const int32_t *landmark, int32_t M, double *err_node, double *nees, int32_t *info, double *err_global,
                    viekf_mem where);

#ifdef __cplusplus
}
#endif

#endif /* VIEKF_MAP_H */
