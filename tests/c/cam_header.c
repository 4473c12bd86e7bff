/* include/viekf_cam.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has every entry point refuse a null handle and the defaults set. */
#include <stdio.h>
#include <string.h>

#include "viekf_cam.h"

int main(void) {
  viekf_cam *c = NULL;
  viekf_cam_intrinsics k;
  int bad = 0;
  bad += viekf_cam_create(0, 0, &c) != VIEKF_ERR_INVALID || c != NULL;
  bad += viekf_cam_create(1, 0, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_destroy(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_dims(NULL, NULL, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_set_stream(NULL, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_sync(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_set_intrinsics(NULL, NULL, 0) != VIEKF_ERR_INVALID;
  bad += viekf_cam_get_intrinsics(NULL, NULL, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_distort_points(NULL, 1, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_cam_undistort_points(NULL, 1, NULL, NULL, 0, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_cam_valid_mask(NULL, 8, 8, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_cam_warp(NULL, VIEKF_CAM_RECTIFY, 8, 8, NULL, NULL, NULL, NULL, 0, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += viekf_cam_intrinsics_default(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_cam_load_yaml(NULL, NULL, &k) != VIEKF_ERR_INVALID;
  bad += viekf_cam_intrinsics_default(&k) != VIEKF_OK;
  bad += k.focal[0] != 1.0 || k.focal[1] != 1.0 || k.out_focal[0] != 1.0 || k.out_focal[1] != 1.0;
  bad += k.center[0] != 0.0 || k.out_center[1] != 0.0 || k.dist[0] != 0.0 || k.dist[3] != 0.0 || k.min_det != 0.0;
  bad += sizeof(viekf_cam_intrinsics) != 13 * sizeof(double);
  bad += VIEKF_CAM_MAX_ITER != 20 || VIEKF_CAM_SCAN_DIRS != 32 || VIEKF_CAM_SCAN_STEP * 256.0 != 1.0 || VIEKF_CAM_SCAN_CAP != 4.0;
  bad += VIEKF_CAM_OK != 0 || VIEKF_CAM_PADDING != 1 || VIEKF_CAM_OUT_OF_MODEL != 2;
  if (bad) {
    fprintf(stderr, "cam header check failed: %d\n", bad);
    return 1;
  }
  printf("cam header ok\n");
  return 0;
}
