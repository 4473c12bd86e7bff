/* include/viekf_body.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has the entry point refuse a null handle and the layout function answer. */
#include <stdio.h>
#include <string.h>

#include "viekf_body.h"

int main(void) {
  int bad = 0;
  int32_t types[1] = {VIEKF_POS}, zdim[1] = {3}, rdim[1] = {3}, route = -7;
  double z[4] = {0.0, 0.0, 0.0, 0.0}, R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  bad += viekf_batch_update_body(NULL, 1, types, zdim, rdim, z, R, 0, NULL, NULL, &route, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += route != -7;
  bad += VIEKF_BODY_MAX_M != 8;
  /* 8 (nx' + 18 n + N + 6 n M + 64) at N = 50: nx' = 268, n = 166 */
  bad += viekf_body_lds_bytes(50, 2) != 8 * (268 + 18 * 166 + 50 + 6 * 166 * 2 + 64);
  bad += viekf_body_lds_bytes(50, 0) != 0 || viekf_body_lds_bytes(50, VIEKF_BODY_MAX_M + 1) != 0;
  bad += viekf_body_lds_bytes(50, VIEKF_BODY_MAX_M) > 160 * 1024;
  bad += viekf_body_lds_limit(0, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_abi_version() != 1;
  if (bad) {
    fprintf(stderr, "body header check failed: %d\n", bad);
    return 1;
  }
  printf("body header ok\n");
  return 0;
}
