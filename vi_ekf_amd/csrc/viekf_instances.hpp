// viekf_instances.hpp -- which instances of the fused-step kernels the library holds, and in which translation unit each is
// compiled (viekf_inst.hip, built once per group with -DVIEKF_INST_GROUP=g, in parallel).  viekf_capi.hip sees every instance
// as an `extern template`: it takes their addresses and launches them, the code lives in the group's object file.  The rows
// themselves are written once, in viekf_instance_rows.hpp.
#pragma once
#include "viekf_instance_rows.hpp"
#include "viekf_kernels_resident.hpp"
#include "viekf_kernels_tiles.hpp"

#define VIEKF_STEP_ARGS                                                                                                  \
  viekf::StreamArgs, int, const double*, const double*, const double*, const int*, int, int, const double*, long, long, int*

// (four flavours of a resident instance: several propagates per launch or one; unit-Lambda or general.  Two of a tile
//  instance and two of its pair form.  The rows carry more than the template arguments: the rest is the dispatch table's.)
#define VIEKF_RES_FLAVOURS(PFX, RB, NW, NS, ...)                                                        \
  PFX template __global__ void viekf::k_step_resident<RB, NW, false, NS, false>(VIEKF_STEP_ARGS);  \
  PFX template __global__ void viekf::k_step_resident<RB, NW, false, NS, true>(VIEKF_STEP_ARGS);   \
  PFX template __global__ void viekf::k_step_resident<RB, NW, true, NS, false>(VIEKF_STEP_ARGS);   \
  PFX template __global__ void viekf::k_step_resident<RB, NW, true, NS, true>(VIEKF_STEP_ARGS);
#define VIEKF_TILE_FLAVOURS(PFX, NT, NW, ...)                                            \
  PFX template __global__ void viekf::k_step_tiles<NT, NW, false>(VIEKF_STEP_ARGS);  \
  PFX template __global__ void viekf::k_step_tiles<NT, NW, true>(VIEKF_STEP_ARGS);   \
  PFX template __global__ void viekf::k_step_tiles_pair<NT, false>(VIEKF_STEP_ARGS); \
  PFX template __global__ void viekf::k_step_tiles_pair<NT, true>(VIEKF_STEP_ARGS);
