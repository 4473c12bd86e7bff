/* include/viekf_map.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has every entry point refuse a null handle. */
#include <stdio.h>
#include <string.h>

#include "viekf_map.h"

int main(void) {
  viekf_map *m = NULL;
  int bad = 0;
  bad += viekf_map_create(NULL, NULL, NULL, 0, &m) != VIEKF_ERR_INVALID || m != NULL;
  bad += viekf_map_create(NULL, NULL, NULL, 0, NULL) != VIEKF_ERR_INVALID;
  bad += viekf_map_destroy(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_map_reset(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_map_landmarks(NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_map_update(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_map_get(NULL, NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_map_set(NULL, NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_map_error(NULL, NULL, 0, 1, NULL, NULL, 1, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += VIEKF_MAP_MAX_CAPACITY != 4096;
  if (bad) {
    fprintf(stderr, "map header check failed: %d\n", bad);
    return 1;
  }
  printf("map header ok\n");
  return 0;
}
