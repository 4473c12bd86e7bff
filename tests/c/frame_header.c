/* include/viekf_frame.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has every entry point refuse a null handle. */
#include <stdio.h>
#include <string.h>

#include "viekf_frame.h"

int main(void) {
  viekf_frame *f = NULL;
  int bad = 0;
  bad += viekf_frame_create(NULL, &f) != VIEKF_ERR_INVALID || f != NULL;
  bad += viekf_frame_destroy(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_frame_reset(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_frame_set_tracked(NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_frame_tracked(NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_frame_intake(NULL, 1, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += VIEKF_FRAME_MAX_M != 4096;
  if (bad) {
    fprintf(stderr, "frame header check failed: %d\n", bad);
    return 1;
  }
  printf("frame header ok\n");
  return 0;
}
