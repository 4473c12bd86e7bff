/* include/viekf_node.h is plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links against
 * libviekf_hip.so and, without touching a device, has every entry point refuse a null handle. */
#include <stdio.h>
#include <string.h>

#include "viekf_node.h"

int main(void) {
  viekf_node *nd = NULL;
  int bad = 0;
  bad += viekf_node_create(NULL, 0, &nd) != VIEKF_ERR_INVALID || nd != NULL;
  bad += viekf_node_destroy(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_node_reset(NULL) != VIEKF_ERR_INVALID;
  bad += viekf_node_update(NULL, NULL, NULL, NULL, 0, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_node_global(NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_node_relative_truth(NULL, NULL, NULL, 17, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_node_global_error(NULL, NULL, 17, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_node_get(NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_node_set(NULL, NULL, NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += viekf_node_trail(NULL, NULL, NULL, VIEKF_HOST) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += VIEKF_NODE_MAX_TRAIL != 4096;
  if (bad) {
    fprintf(stderr, "node header check failed: %d\n", bad);
    return 1;
  }
  printf("node header ok\n");
  return 0;
}
