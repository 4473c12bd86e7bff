// viekf_kernels_frame.hpp -- the device-resident frame intake (include/viekf_frame.h): the feature-id
// bookkeeping of VIEKF_ROS::color_image_callback (reference src/vi_ekf_ros.cpp:276-305) as kernels, so that a frame's
// (z, ids) in device memory become the keep / mask / slot arrays the numeric kernels take without a trip to the host.
//
//   k_frame_plan      one wave64 per filter.  The frame's id row and the filter's id table sit in LDS; ids are matched
//                     lane-parallel (a lane per entry, the other side read as an LDS broadcast), 64-bit ballots and
//                     __popcll prefix counts order what comes out: the keep mask and the compacted table, the overlap with
//                     the keyframe list and the reset mask, the new keyframe list, rank and slot of every new feature, and
//                     the REVERSED, front-compacted update arrays slot_u / z_u (R_u for r_mode 2) with the permutation
//                     back to frame order.  The table is committed here: whether an init finds room is len_kept + rank < N.
//   k_init_features   one workgroup per filter: all of a filter's new features in one launch, bit for bit what the same
//                     number of k_init_feature launches leave.
//   k_frame_finish    one wave64 per filter: the update results back in frame order, merged with the codes the plan
//                     decided, the gated list, did_reset.
//   k_frame_slot_plan the id -> slot lookup of the intake's DEPTH and PIXEL_VEL steps, which run behind the intake.
// Between them run the existing k_keep_features, k_keyframe_reset and the batch's own FEAT update.  Synchronisation is
// __syncthreads() and wave intrinsics only: no flags, tickets or polling between waves, nothing here can wait for ever.
#pragma once
#include "viekf_kernel_args.hpp"

namespace viekf {

constexpr int FR_UPDATE = 100;   // plan code of an entry that is one of the frame's updates (never handed out)

// the intake's device tables (all [B] rows; M-sized rows have capacity mcap >= M and are addressed with stride M)
struct FrameTabs {
  int* tab;              // [B][N]  global id of the feature in slot f, -1 past the filter's features
  int* tlen;             // [B]     the table's length: equals len_features unless somebody edited the features elsewhere
  int* kf;               // [B][kfcap] keyframe list
  int* kflen;            // [B]
  int kfcap;
  unsigned char* keep;   // [B][N]  for k_keep_features
  unsigned char* rmask;  // [B]     for k_keyframe_reset
  int* newcnt;           // [B]     features k_init_features starts
  double* newpix;        // [B][N][2]
  double* newdepth;      // [B][N]
  int* code;             // [B][M]  viekf_meas_result decided by the plan, or FR_UPDATE
  int* pos;              // [B][M]  where in the update arrays entry i went (-1: nowhere)
  int* slot_u;           // [B][M]  the update arrays: reverse frame order, compacted to the front, -1 after them
  double* z_u;           // [B][M][2]
  double* R_u;           // [B][M][4] (r_mode 2)
  int* res_u;            // [B][M]
};

__device__ __forceinline__ int fr_prefix(unsigned long long bal, int lane) { return __popcll(bal & ((1ull << lane) - 1ull)); }

// dynamic LDS: int[2 M + 2 N]
__global__ __launch_bounds__(64) void k_frame_plan(StreamArgs a, FrameTabs t, int M, const double* __restrict__ z_all,
                                                   const int* __restrict__ ids_all, const double* __restrict__ depth_all,
                                                   const double* __restrict__ R_all, int r_mode,
                                                   const unsigned char* __restrict__ active, int use_kfr, double thresh,
                                                   double* __restrict__ edges) {
  extern __shared__ int fsm[];
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= a.B) return;
  const int N = a.N;
  int* ids = fsm;       // [M] the frame's ids; from pass D on the slot of an update entry
  int* st = ids + M;    // [M] -1 skipped, 3 repeat, 0 pending, then 2 / 4 / FR_UPDATE + rank among the updates
  int* tab = st + M;    // [N] the table as it was
  int* aux = tab + N;   // [N] the table as it will be
  const long bM = (long)b * M, bN = (long)b * N;
  const int tl = min(max(t.tlen[b], 0), N);
  const bool act = !active || active[b];
  const bool stale = a.len[b] != tl;
  if (edges && lane < 17) edges[(long)b * 17 + lane] = 0.0;
  for (int i = lane; i < M; i += 64) ids[i] = ids_all[bM + i];
  for (int f = lane; f < N; f += 64) tab[f] = t.tab[bN + f];
  __syncthreads();
  if (!act || stale) {   // nothing of the filter or the table changes
    for (int i = lane; i < M; i += 64) {
      t.code[bM + i] = (!act || ids[i] < 0) ? -1 : 3;
      t.pos[bM + i] = -1; t.slot_u[bM + i] = -1; t.res_u[bM + i] = -1;
      t.z_u[2 * (bM + i)] = 0.0; t.z_u[2 * (bM + i) + 1] = 0.0;
      if (r_mode == 2) for (int q = 0; q < 4; q++) t.R_u[4 * (bM + i) + q] = 0.0;
    }
    for (int f = lane; f < N; f += 64) t.keep[bN + f] = 1;
    if (lane == 0) { t.rmask[b] = 0; t.newcnt[b] = 0; }
    return;
  }
  // A: repeats.  Entry i repeats an id if an earlier entry holds it (the first one counts, whatever its z)
  for (int i0 = 0; i0 < M; i0 += 64) {
    const int i = i0 + lane, id = i < M ? ids[i] : -1, jmax = min(i0 + 64, M);
    bool dup = false;
    for (int j = 0; j < jmax; j++) dup |= (j < i && ids[j] == id);
    if (i < M) st[i] = id < 0 ? -1 : (dup ? 3 : 0);
  }
  // B: which tracked ids the frame still holds; their new slots; the overlap with the keyframe list
  const int kfl = min(max(t.kflen[b], 0), t.kfcap);
  int* kfrow = t.kf + (long)b * t.kfcap;
  int len_kept = 0, overlap = 0;
  for (int f0 = 0; f0 < N; f0 += 64) {
    const int f = f0 + lane, id = f < tl ? tab[f] : -1;
    bool present = false, inkf = false;
    if (f0 < tl) {
      for (int j = 0; j < M; j++) present |= ids[j] == id;
      for (int j = 0; j < kfl; j++) inkf |= kfrow[j] == id;
    }
    present = present && f < tl && id >= 0;
    const unsigned long long bal = __ballot(present);
    if (present) aux[len_kept + fr_prefix(bal, lane)] = id;
    if (f < N) t.keep[bN + f] = present ? 1 : 0;
    len_kept += __popcll(bal);
    overlap += __popcll(__ballot(present && inkf));
  }
  __syncthreads();
  // C: the keyframe test (vi_ekf_feat.cpp:119-139), the quotient in double as the reference forms it
  const bool do_reset = use_kfr && kfl > 0 && (double)overlap / (double)kfl < thresh;
  if (do_reset || (use_kfr && kfl == 0)) {   // list := the frame's ids
    int cnt = 0;
    for (int i0 = 0; i0 < M; i0 += 64) {
      const int i = i0 + lane;
      const bool v = i < M && st[i] == 0;
      const unsigned long long bal = __ballot(v);
      const int at = cnt + fr_prefix(bal, lane);
      if (v && at < t.kfcap) kfrow[at] = ids[i];
      cnt += __popcll(bal);
    }
    if (lane == 0) t.kflen[b] = min(cnt, t.kfcap);
  }
  if (lane == 0) t.rmask[b] = do_reset ? 1 : 0;
  // D: every pending entry is a NaN, a new feature or an update
  const int room = N - len_kept;
  int nnew = 0, nupd = 0;
  for (int i0 = 0; i0 < M; i0 += 64) {
    const int i = i0 + lane;
    const bool pend = i < M && st[i] == 0;
    const int id = pend ? ids[i] : -1;
    double z0 = 0.0, z1 = 0.0;
    if (pend) { z0 = z_all[2 * (bM + i)]; z1 = z_all[2 * (bM + i) + 1]; }
    const bool nan = pend && (z0 != z0 || z1 != z1);
    int slot = -1;
    for (int j = 0; j < len_kept; j++) slot = (aux[j] == id) ? j : slot;
    const bool isnew = pend && !nan && slot < 0, isupd = pend && !nan && slot >= 0;
    const unsigned long long bn = __ballot(isnew), bu = __ballot(isupd);
    if (isnew) {
      const int rank = nnew + fr_prefix(bn, lane);
      if (rank < room) {   // init_feature will find a slot: the id joins the table now
        aux[len_kept + rank] = id;
        t.newpix[2 * (bN + rank)] = z0; t.newpix[2 * (bN + rank) + 1] = z1;
        t.newdepth[bN + rank] = depth_all ? depth_all[bM + i] : NAN;
      }
      st[i] = 4;
    } else if (isupd) {
      st[i] = FR_UPDATE + nupd + fr_prefix(bu, lane);
      ids[i] = slot;
    } else if (nan) st[i] = 2;
    nnew += __popcll(bn); nupd += __popcll(bu);
  }
  __syncthreads();
  const int ninit = min(nnew, room), tl_new = len_kept + ninit;
  for (int f = lane; f < N; f += 64) t.tab[bN + f] = f < tl_new ? aux[f] : -1;
  if (lane == 0) { t.tlen[b] = tl_new; t.newcnt[b] = ninit; }
  // the update arrays: reverse frame order (the reference's queue, vi_ekf_meas.cpp:150-176), compacted to the front
  for (int i = lane; i < M; i += 64) {
    const int c = st[i];
    int p = -1;
    if (c >= FR_UPDATE) {
      p = nupd - 1 - (c - FR_UPDATE);
      t.slot_u[bM + p] = ids[i];
      t.z_u[2 * (bM + p)] = z_all[2 * (bM + i)]; t.z_u[2 * (bM + p) + 1] = z_all[2 * (bM + i) + 1];
      if (r_mode == 2) for (int q = 0; q < 4; q++) t.R_u[4 * (bM + p) + q] = R_all[4 * (bM + i) + q];
    }
    t.code[bM + i] = c >= FR_UPDATE ? FR_UPDATE : c;
    t.pos[bM + i] = p;
    t.res_u[bM + i] = -1;
    if (i >= nupd) {
      t.slot_u[bM + i] = -1;
      t.z_u[2 * (bM + i)] = 0.0; t.z_u[2 * (bM + i) + 1] = 0.0;
      if (r_mode == 2) for (int q = 0; q < 4; q++) t.R_u[4 * (bM + i) + q] = 0.0;
    }
  }
}

// init_feature (vi_ekf_feat.cpp:6-47) for newcnt[b] features of filter b at once: feature k takes slot len + k, its state from
// newpix / newdepth [B][N] row b entry k.  Writes exactly the elements k_init_feature writes, call after call: the strips and
// blocks of different new features never meet (a strip of feature k ends at column 16 + 3 (len + k), where its block starts).
template <int T>
__global__ __launch_bounds__(T) void k_init_features(StreamArgs a, const int* __restrict__ newcnt, const double* __restrict__ newpix,
                                                     const double* __restrict__ newdepth) {
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= a.B) return;
  const int len = a.len[b];
  if (len < 0 || len >= a.N) return;   // :9-10
  const int cnt = min(newcnt[b], a.N - len);
  if (cnt <= 0) return;
  const int n = a.n, ld = a.ld;
  double* P = a.P + a.si(b) * n * ld;
  const long bN = (long)b * a.N;
  for (int k = tid; k < cnt; k += T) {
    double q[4], rho;
    init_feature_state(newpix + 2 * (bN + k), newdepth[bN + k], a.prm(b), q, &rho);
    double* xf = a.x + a.si(b) * a.nxs + xZ + 5 * (len + k);
    xf[0] = q[0]; xf[1] = q[1]; xf[2] = q[2]; xf[3] = q[3]; xf[4] = rho;
  }
  for (int k = 0; k < cnt; k++) {
    const int d0 = 16 + 3 * (len + k);
    for (int e = tid; e < 3 * d0; e += T) {   // zero the cross strips, set the 3x3 block to P0_feat (:39-42)
      const int j = e / 3, r = e % 3;
      P[(d0 + r) + (long)j * ld] = 0.0;
      P[j + (long)(d0 + r) * ld] = 0.0;
    }
    if (tid < 9) {
      const int r = tid % 3, c = tid / 3;
      P[(d0 + r) + (long)(d0 + c) * ld] = (r == c) ? a.prm(b).P0_feat[r] : 0.0;
    }
  }
  __syncthreads();
  if (tid == 0) a.len[b] = len + cnt;
}

// results in frame order, the gated list, did_reset.  Every output may be NULL.
__global__ __launch_bounds__(64) void k_frame_finish(int B, FrameTabs t, int M, const int* __restrict__ ids_all, int* __restrict__ result,
                                                     int* __restrict__ gated, int* __restrict__ gated_count,
                                                     unsigned char* __restrict__ did_reset) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  const long bM = (long)b * M;
  int ng = 0;
  for (int i0 = 0; i0 < M; i0 += 64) {
    const int i = i0 + lane;
    int r = -1;
    bool g = false;
    if (i < M) {
      const int c = t.code[bM + i], p = t.pos[bM + i];
      r = (c == FR_UPDATE && p >= 0 && p < M) ? t.res_u[bM + p] : c;
      g = c == FR_UPDATE && r == 1;
      if (result) result[bM + i] = r;
    }
    const unsigned long long bal = __ballot(g);
    if (g && gated) gated[bM + ng + fr_prefix(bal, lane)] = ids_all[bM + i];
    ng += __popcll(bal);
  }
  if (gated) for (int i = ng + lane; i < M; i += 64) gated[bM + i] = -1;
  if (lane == 0) {
    if (gated_count) gated_count[b] = ng;
    if (did_reset) did_reset[b] = t.rmask[b];
  }
}

// viekf_frame_intake_depth / viekf_frame_intake_pixel_vel: which entries of a frame are measurements of the step's kind, and
// their slots.  One workgroup of 64 per filter; val [B][M][ZD] is what an entry measures (a depth: ZD = 1, a flow: 2).
//   slot_out [B][M]: the slot of the entry's id in the intake's table; -1 (the update answers SKIPPED) for an entry that is no
//   measurement or a filter without a frame; kFrameNoSlot (>= every len_features: INVALID) for an id that is not in the table,
//   and for every id >= 0 of a filter whose table is stale.   act_out [B][M]: use.
constexpr int kFrameNoSlot = 0x7fffffff;
template <int ZD>
__global__ __launch_bounds__(64) void k_frame_slot_plan(int B, int N, int M, const int* __restrict__ len, const int* __restrict__ tab,
                                                        const int* __restrict__ tlen, const int* __restrict__ ids,
                                                        const double* __restrict__ val, const int* __restrict__ feat_result,
                                                        const unsigned char* __restrict__ active, int use, int* __restrict__ slot_out,
                                                        unsigned char* __restrict__ act_out) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const bool act = active ? active[b] != 0 : true;
  const int tl = tlen[b];
  const bool stale = len[b] != tl;
  const int* row = tab + (long)b * N;
  for (int i = threadIdx.x; i < M; i += 64) {
    const long at = (long)b * M + i;
    const int id = ids[at];
    int slot = -1;
    if (act && id >= 0) {
      if (stale) slot = kFrameNoSlot;
      else {
        const int fr = feat_result[at];
        bool finite = true;   // (false for a NaN)
        for (int q = 0; q < ZD; q++) finite &= fabs(val[ZD * at + q]) <= 1.7976931348623157e308;
        if ((fr == 0 || fr == 1) && finite) {   // queued as FEAT, finite measurement
          slot = kFrameNoSlot;
          for (int f = 0; f < tl && f < N; f++)
            if (row[f] == id) { slot = f; break; }
        }
      }
    }
    slot_out[at] = slot;
    act_out[at] = use ? (unsigned char)1 : (unsigned char)0;
  }
}

// viekf_frame_set_tracked: a row's length is the number of its leading ids >= 0; what follows becomes -1
__global__ __launch_bounds__(64) void k_frame_adopt(int B, int N, int* __restrict__ tab, int* __restrict__ tlen) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= B) return;
  int* row = tab + (long)b * N;
  int len = N;
  for (int f0 = 0; f0 < N && len == N; f0 += 64) {
    const int f = f0 + lane;
    const unsigned long long neg = __ballot(f < N && row[f] < 0);
    if (neg) len = f0 + __ffsll((long long)neg) - 1;
  }
  for (int f = len + lane; f < N; f += 64) row[f] = -1;
  if (lane == 0) tlen[b] = len;
}

}  // namespace viekf
