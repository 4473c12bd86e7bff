/* include/viekf_depth.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has the entry points refuse a null handle and the layout function answer. */
#include <stdio.h>
#include <string.h>

#include "viekf_depth.h"

int main(void) {
  int bad = 0;
  int32_t slot[2] = {0, 1}, route = -7, res[2] = {9, 9};
  double z[2] = {3.0, 3.0}, R[1] = {0.01};
  bad += viekf_batch_update_depths(NULL, VIEKF_DEPTH, 2, slot, z, R, 0, NULL, 0, res, &route, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += route != -7 || res[0] != 9;
  bad += viekf_frame_intake_depth(NULL, 2, slot, z, slot, R, 0, 1, NULL, res, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += VIEKF_DEPTHS_MAX_M < 256;
  /* 8 (even(nx' + n + N) + 2 + even(M) + n' M) at N = M = 50: nx' = 268, n = n' = 166 */
  bad += viekf_depths_lds_bytes(50, 50) != 8 * (268 + 166 + 50 + 2 + 50 + 166 * 50);
  /* N = 5, M = 3: nx' = 42, n = 31, n' = 32: even(78) + 2 + even(3) + 96 */
  bad += viekf_depths_lds_bytes(5, 3) != 8 * (78 + 2 + 4 + 32 * 3);
  bad += viekf_depths_lds_bytes(50, 0) != 0 || viekf_depths_lds_bytes(50, VIEKF_DEPTHS_MAX_M + 1) != 0;
  bad += viekf_depths_lds_bytes(-1, 1) != 0;
  bad += 2 * viekf_depths_lds_bytes(50, 50) > 160 * 1024; /* two workgroups per compute unit at the headline size */
  bad += viekf_depths_lds_bytes(77, 77) > 160 * 1024;
  bad += viekf_abi_version() != 1;
  if (bad) {
    fprintf(stderr, "depth header check failed: %d\n", bad);
    return 1;
  }
  printf("depth header ok\n");
  return 0;
}
