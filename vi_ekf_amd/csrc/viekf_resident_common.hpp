// viekf_resident_common.hpp -- resident (fused-step) kernel family: shared launch state and the small device helpers both roles
// use.  The LDS carve-up (ResLds), the words of the scratchpad S.sm (res_sm) and the launch word: viekf_fused_lds.hpp.  Overview of
// the family: viekf_kernels_resident.hpp.
#pragma once
#include <type_traits>

#include "viekf_fused_lds.hpp"
#include "viekf_instance_rows.hpp"
#include "viekf_kernel_args.hpp"

namespace viekf {

#ifndef RES_INLINE
#define RES_INLINE __forceinline__
#endif
// ------------------------------------------------------------------------------------------------
// fused step: [propagate] + M feature updates with P resident in registers, WARP-SPECIALISED:
//   worker waves (NW x 64 threads) own P and run only the lean contraction / sweep code;
//   one service wave runs the scalar-heavy math (dynamics, gain, manifold correction, h_feat).
// Both sides execute the same barrier sequence; their register footprints never mix, which is
// what keeps the sweep loops spill-free (a spill costs a ~1 us scratch round trip per use).
// ------------------------------------------------------------------------------------------------
// Returns v unchanged but opaque to the optimiser: values derived from it cannot be hoisted out of a loop and kept
// (or spilled) across iterations; recomputing a few integer ops per use is far cheaper than a scratch round trip.
// Orders LDS accesses of DIFFERENT lanes of one wave: a store under a lane predicate followed by loads on other lanes.  The
// hardware executes one wave's LDS instructions in order, but lanes are separate threads to the compiler, which otherwise
// hoists the other lanes' loads above the predicated store.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int opaque(int v) { asm volatile("" : "+v"(v)); return v; }
// Many blocks per thread: fences the operand loads of one group of blocks from the next (a compiler-level memory barrier plus
// a scheduling barrier) -- otherwise every block's (mutually independent) LDS reads are hoisted to the top and their results
// held live together, which does not fit the register file next to the blocks themselves.
// 16-byte LDS read as ONE vector load: through HIP's double2 struct the two halves are often split and re-paired as
// ds_read2_b64 (8 LDS cycles per wave instruction, 32-bank mapping) instead of ds_read_b128 (4 cycles, 64 banks)
typedef double v2f64 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double2 lds_ld2(const double* p) {
  const v2f64 v = *reinterpret_cast<const v2f64*>(p);
  return make_double2(v.x, v.y);
}
template <bool ON>
__device__ __forceinline__ void group_fence() {
  if (ON) {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
  }
}
__device__ __forceinline__ double uniform_f64(double v) {   // force a wave-uniform double into SGPRs
  const unsigned long long u = __double_as_longlong(v);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u), hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
  return __longlong_as_double(((unsigned long long)hi << 32) | lo);
}

// Diagnostic build only (-DVIEKF_STAMPS): s_memtime stamps of block 0 into the (otherwise unused) workspace.
// (-DVIEKF_STAMPS=2 keeps only the per-wave stamps of one update, 192 .. 223: thread 0's per-update stamps are then not in wave 0's
//  instruction stream -- an s_memtime in flight turns that wave's counted LDS waits into full drains, NOTES A (xix) -- and the three
//  worker waves run the same code)
#ifdef VIEKF_STAMPS
#if VIEKF_STAMPS + 0 == 2
#define RES_STAMP_KEPT(idx) ((idx) >= 192 && (idx) < 224)
#else
#define RES_STAMP_KEPT(idx) true
#endif
#define RES_STAMP(S_, who, idx)                                                                  \
  do {                                                                                           \
    if (RES_STAMP_KEPT(idx) && (S_).b == 0 && (who)) {                                                                  \
      __builtin_amdgcn_sched_barrier(0);                                                         \
      reinterpret_cast<unsigned long long*>((S_).stamps)[(idx)] = __builtin_amdgcn_s_memtime();  \
      __builtin_amdgcn_sched_barrier(0);                                                         \
    }                                                                                            \
  } while (0)
#else
#define RES_STAMP(S_, who, idx) do {} while (0)
#endif

// Accounting build only (-DVIEKF_ISA_MARKS, tools/isa_regions.py): named marks in the ISA listing, fenced so that nothing is
// scheduled across them -- the per-region instruction counts of profiles/r03/isa_step_resident_7_3.json.
#ifdef VIEKF_ISA_MARKS
#define RES_MARK(name)                          \
  do {                                          \
    __builtin_amdgcn_sched_barrier(0);          \
    asm volatile("; @@MARK " name);             \
    __builtin_amdgcn_sched_barrier(0);          \
  } while (0)
#else
#define RES_MARK(name) do {} while (0)
#endif

// Timing-only ablation bits (results become wrong) exist in a -DVIEKF_ABLATE diagnostic build only; the product build has none.
#ifdef VIEKF_ABLATE
#define RES_ABLATE(S_, bit) (((S_).dbg & (bit)) != 0)
#else
#define RES_ABLATE(S_, bit) false
#endif

typedef __attribute__((address_space(3))) volatile int lds_vint_t;

struct ResShared {  // resolved LDS pointers + launch constants shared by both roles
  double *xs, *Kt, *Wt, *Praw, *lam, *sm, *fixadd, *fixset, *Z, *phiff, *Abb, *Gb, *Phibb, *Mbb, *Gdb, *Pbb, *T16,
      *xdb, *Pbc, *PhibbT, *Pd, *PsiP, *Pi, *Xi, *AvG, *Lbc, *mz, *mR;
  int* mslot;   // [res_mcap(N)] slot, or -1 for a measurement that is not run
  int2* mseq;   // [res_mcap(N)] {index of the next measurement that runs (or M), its slot (or -1)}: one LDS read per iteration
  BodyCtx* ctx;
  int N, n, nf, len, M, mstride, do_prop, b, dbg, kp, B, img_len, mcap;   // kp: propagates per launch (viekf_batch_step_n)
  int fmt;      // RES_FMT_* bits of this launch
  long si, so;   // the filter's entry of x / P it is loaded from and stored to (StreamArgs::si / so, read ONCE in the prologue)
  double* stamps;
};

// Ownership words of worker thread t (build_resmap, viekf_resmap.cpp: entry [slot][t] = I | J << 8 | owned << 16).  A use site
// loads ALL of its thread's words in one batch and decodes them in registers: a load per block, each waited for before the block's
// own loads or LDS reads may issue, is one exposed memory round trip per block (7 in a row at 7 blocks per thread).
template <int RB, int TW>
__device__ __forceinline__ void res_words(const int* __restrict__ resmap, int t, int (&w)[RB]) {
#pragma unroll
  for (int ia = 0; ia < RB; ia++) w[ia] = resmap[ia * TW + t];
}
// (which instances do so, and stage sqrt(Qu) / Qx in LDS: res_batched_loads, viekf_fused_lds.hpp)
// Which instances spread the block loads of P over the propagate's set-up and first wait for them behind B3p (res_worker, switch
// SU): the single-propagate kernels of <4,3>, <6,3>, <7,3> and <5,6> -- the instances that timed faster or equal with it, each
// against the parent (profiles/setup_under_load/instances_ab.md).  <2,1>, <2,2>, <3,2> (two or three blocks per thread: little to
// spread, one more batch of address arithmetic) measured 1 - 5 % SLOWER, <5,3> and <7,6> slower beyond their spread in the
// unit-Lambda step (+1.4 %, +0.5 %): they keep the old order.  So do the multi-propagate kernels -- their set-up reads sqrt(Qu) from
// memory, a vector load that would drain the blocks, and only the first of K trips has loads in flight -- and <6,6> at the register
// file's end (254 VGPRs: with its blocks in flight across the set-up, all issued ahead of B0, its unit-Lambda kernel spilled two
// registers to scratch; the spread form was not tried on it).  An instance that keeps the old order compiles to the instruction
// stream it had before.
constexpr bool res_setup_under_load(int RB, int NW, bool MP) {
  return res_batched_loads(RB, NW) && !MP && ((NW == 3 && (RB == 4 || RB == 6 || RB == 7)) || (NW == 6 && RB == 5));
}
// Which kernels run the BODY-ONLY part of the propagate's set-up on the service wave (res_prop_setup_body_service,
// viekf_resident_prop.hpp): Phi_bb / M_bb, Psi P_bb, T16, Gs_b, Pi and Xi involve the 16 x 16 body blocks alone, and between B1p and
// B3p the service wave of a single-propagate kernel has nothing to do but the body state step and fix_depth.  With the gate on the
// workers keep the expansion of the feature rows and V ([B1p..B2p]) and the Ut product ([B2p..B3p]); the barrier B2q is gone.  Every
// element is the same expression on the same operands, so the results are bit for bit those of the old order.  The gate
// covers the single-propagate kernels that run the set-up under the load (res_setup_under_load): there the workers reach B0 idle
// and B3p is set by dynamics plus set-up -- <6,3>, <7,3> and <5,6>; <4,3> is gated off: its unit-Lambda step measured 1.0 % SLOWER,
// beyond its spread, with its general-Lambda step and its propagate-only launch 0.7 - 1.0 % faster
// (profiles/service_setup/instances_ab.md).  The multi-propagate kernels keep the old order -- their service wave fills this time
// with the next propagate's body dynamics.  VIEKF_SERVICE_SETUP=0 at build time gives every kernel the old order, and a kernel
// whose gate is off compiles to the instruction stream it had before.  VIEKF_SERVICE_SETUP_CHUNKS: where the third chunk of the
// block loads is issued in the shorter set-up -- 1: behind a wave's first turn of the Ut product (the default: the headline step
// measured -1.8 % against the parent with it, -1.2 % with 0), 0: behind B2p with the second (18 + 36 loads at 7 blocks per thread).
#ifndef VIEKF_SERVICE_SETUP
#define VIEKF_SERVICE_SETUP 1
#endif
#ifndef VIEKF_SERVICE_SETUP_CHUNKS
#define VIEKF_SERVICE_SETUP_CHUNKS 1
#endif
constexpr bool res_service_setup(int RB, int NW, bool MP) {
  return (VIEKF_SERVICE_SETUP) != 0 && res_setup_under_load(RB, NW, MP) && RB != 4;
}
// Which kernels ROTATE the operand reads of their sweeps under the multiply-adds (res_worker), a mask of parts:
//   1  the update loop's block sweep: two operand buffers, block ia + 2's rows of K and W are read into the buffer block ia's
//      multiply-adds just released -- L(0) L(1) F(0) L(2) F(1) ... F(RB - 1) -- instead of two blocks' reads, a wait, their
//      multiply-adds and a fence, four times per update at RB = 7.  A gated or NaN-guarded update reads no operand
//   2  the propagate's K = 24 contraction, the same order inside a trip k
// Only instances with more than four blocks per thread have groups to rotate (RB <= 4 holds every operand in flight at once); all
// seven of them take both parts, in every flavour: no launch of theirs timed slower beyond its spread, none gained a spill
// (profiles/rotating_reads/instances_ab.md, budget.md) -- the arguments beyond RB are there for an instance that has to be gated off.
// VIEKF_ROTATING_READS masks the parts at build time (tools/build_variant.sh parent_order -DVIEKF_ROTATING_READS=0 builds the
// old order from this tree); a kernel whose mask is 0 compiles to the instruction stream it had before.
#ifndef VIEKF_ROTATING_READS
#define VIEKF_ROTATING_READS 3
#endif
constexpr int res_rotating_reads(int RB, int NW, bool MP, bool ZU) {
  return (RB > 4) ? ((VIEKF_ROTATING_READS) & 3) : 0;
}
// false = not owned (then I = J = 0: every LDS / global read stays in range, results are never stored)
__device__ __forceinline__ bool res_word_blk(int e, int& I, int& J) {
  I = e & 0xff;
  J = (e >> 8) & 0xff;
  return (e >> 16) != 0;
}

// first m' >= from whose update will actually run (mslot >= 0), else M
__device__ __forceinline__ int res_next_valid(const ResShared& S, int from) {
  int m = from;
  while (m < S.M && S.mslot[m] < 0) m++;
  return m;
}

}  // namespace viekf
