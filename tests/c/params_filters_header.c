/* The per-filter parameter sets of include/viekf.h from plain C11: this program builds with -Wall -Wextra -Werror -pedantic, links
 * against libviekf_hip.so and, without touching a device, holds the two entry points to their declared signatures and has them
 * refuse a null handle. */
#include <stdio.h>
#include <string.h>

#include "viekf.h"

/* the declared signatures: an assignment to these pointer types does not compile (-Werror) against any other */
static int (*const set_fn)(viekf_batch *, const viekf_params *) = viekf_batch_set_params_filters;
static int (*const get_fn)(const viekf_batch *, int32_t, viekf_params *) = viekf_batch_get_params_filter;

int main(void) {
  int bad = 0;
  viekf_params p, q;
  bad += viekf_params_default(&p) != VIEKF_OK;
  q = p;
  bad += set_fn(NULL, &p) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += set_fn(NULL, NULL) != VIEKF_ERR_INVALID;
  bad += get_fn(NULL, 0, &q) != VIEKF_ERR_INVALID;
  bad += strstr(viekf_last_error(), "null") == NULL;
  bad += memcmp(&p, &q, sizeof p) != 0; /* (a refused call writes nothing) */
  bad += viekf_abi_version() != 1 || VIEKF_ABI_VERSION != 1;
  if (bad) {
    fprintf(stderr, "params_filters header check failed: %d\n", bad);
    return 1;
  }
  printf("params_filters header ok\n");
  return 0;
}
