/* include/viekf_pixvel.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has the entry points refuse a null handle and the layout function answer. */
#include <stdio.h>
#include <string.h>

#include "viekf_pixvel.h"

int main(void) {
  int bad = 0;
  int32_t slot[2] = {0, 1}, route = -7, res[2] = {9, 9};
  double z[4] = {3.0, 3.0, 1.0, 1.0}, R[4] = {100.0, 0.0, 0.0, 100.0}, gyro[3] = {0.0, 0.0, 0.0}, dt[1] = {0.04}, out[4] = {7.0, 7.0, 7.0, 7.0};
  bad += viekf_batch_update_pixel_vels(NULL, 2, slot, z, gyro, R, 0, 0.0, NULL, 0, res, &route, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += route != -7 || res[0] != 9;
  bad += viekf_batch_eval_pixel_vel(NULL, slot, gyro, out, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_pixel_flow(NULL, 2, z, slot, 2, z, slot, dt, out, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += out[0] != 7.0;
  bad += viekf_frame_intake_pixel_vel(NULL, 2, slot, z, slot, gyro, R, 0, 0.0, 1, NULL, res, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += VIEKF_PIXVELS_MAX_M < 256 || VIEKF_PIXEL_FLOW_MAX_M < 4096;
  /* 8 (nx' + 5 n + 32) at N = 50: nx' = 268, n = 166 */
  bad += viekf_pixvel_lds_bytes(50) != 8 * (268 + 5 * 166 + 32);
  /* N = 5: nx' = 42, n = 31 */
  bad += viekf_pixvel_lds_bytes(5) != 8 * (42 + 5 * 31 + 32);
  /* 8 (nx' + n' + even(N) + 9 n' + 32 + 4 M + 2 n' M) at N = M = 50 */
  bad += viekf_pixvels_lds_bytes(50, 50) != 8 * (268 + 166 + 50 + 9 * 166 + 32 + 200 + 2 * 166 * 50);
  bad += viekf_pixvels_lds_bytes(50, 50) > 160 * 1024 || viekf_pixvels_lds_bytes(50, 0) != 0;
  bad += viekf_batch_pixel_vels_route(NULL, 0) != VIEKF_ERR_INVALID;
  bad += viekf_pixvel_lds_bytes(-1) != 0 || viekf_pixvel_lds_bytes(4097) != 0;
  bad += viekf_abi_version() != 1;
  if (bad) {
    fprintf(stderr, "pixvel header check failed: %d\n", bad);
    return 1;
  }
  printf("pixvel header ok\n");
  return 0;
}
