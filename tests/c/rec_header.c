/* include/viekf_rec.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has every entry point refuse a null handle. */
#include <stdio.h>
#include <string.h>

#include "viekf_rec.h"

int main(void) {
  viekf_rec *r = NULL;
  int32_t n = 7;
  int bad = 0;
  bad += viekf_rec_create(NULL, 1, 0, &r) != VIEKF_ERR_INVALID || r != NULL;
  bad += viekf_rec_create(NULL, 1, 0, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_rec_destroy(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_rec_reset(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_rec_count(NULL, &n) != VIEKF_ERR_INVALID || n != 7;
  bad += viekf_rec_push(NULL, 0.0, NULL, NULL, 10, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_rec_get(NULL, NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_rec_trajectory_error(NULL, 1, 0, -1, 1, NULL, NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_rec_pose_ensemble(NULL, 0, -1, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_rec_channels(NULL, 0, -1, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += VIEKF_REC_MAX_FRAMES != 4096 || VIEKF_REC_MAX_CHANNELS != 8;
  if (bad) {
    fprintf(stderr, "rec header check failed: %d\n", bad);
    return 1;
  }
  printf("rec header ok\n");
  return 0;
}
