// solve.hip -- the fused HOUV optimisation loop for gfx950 (MI355X).
//
// One workgroup owns one hypothesis (pair p, restart k) for the whole loop:
//   pose from 8 scalars -> move the source cloud -> 4-metric bidirectional Chamfer (two LDS-resident
//   brute-force sweeps) -> top-k robust loss -> closed-form gradient -> Adam step, `n_iters` times,
// with both clouds resident in LDS and NOTHING but the 24-double state touching HBM in between.
// houv_solve_iterate[_pruned] launch one workgroup per hypothesis; houv_solve_stage[_pruned] launch a persistent grid that draws
// (hypothesis, chunk) tickets, each such item being exactly that launch's work for one hypothesis (Stage scheduling).
// It replaces the PyTorch loop of predict_model (registration/models/houv.py:106-138; loss :209-222,
// model_utils_completion.py:83-100,157-166) and of getPredict_angle (registration/train_utils.py:359-456),
// which per iteration launches 8 NmDistanceKernel + 8 NmDistanceGradKernel + 8 topk + ~150 small kernels
// on K-fold replicated clouds.
//
// Design notes (DESIGN.md has the long form):
//   * sweep: every lane owns Q query points in registers; reference points are read from LDS with
//     wave-uniform ds_read_b128 (broadcast), two at a time; the four squared distances (full + three
//     axis-dropped views) share dx,dy,dz: 3 sub + 2 mul + 4 fma + 4 min3/2 = 11 VALU ops per point pair;
//   * arg-min is deferred: a per-32-reference sub-tile id is tracked (3 ops per 32 refs) and the exact
//     NN is recovered by re-evaluating that sub-tile with bit-identical arithmetic;
//   * no distance/index arrays are ever materialised: the epilogue of each sweep turns (NN, dist)
//     straight into the 13 sums the parameter gradient needs (sum sqrt d, sum G, sum G p^T);
//   * top-k (k = N/2 for the full metric) = exact 4-pass 8-bit radix select on the fp32 bit patterns
//     of the register-resident distances, LDS histogram;
//   * the un-moved source point needed for sum G p^T in the target->moved direction is R^T(p' - T);
//   * PRUNE = 0 is that brute-force sweep (north_star's formulation).  PRUNE = 2 / 3 -- the product default for clouds of
//     257..2048 / 2049..4096 points -- replace the two sweeps by the EXACT pruned search of houv_sweep.h (remembered-NN
//     bounds + boxes of k-d-leaf sub-tiles + a balanced, sorted-block walk): same (minimum, sub-tile) per query and metric,
//     hence the same bits everywhere downstream, for ~1/8 of the point pairs.
#include <stddef.h>
#include <stdlib.h>

#include "../../include/houv_hip.h"
#include "houv_common.h"
#include "houv_solve.h"

namespace houv {
namespace {

struct SolveArgs : SolveCommon {
  short* nn_ws;      // pruned mode, per hypothesis 16 rows of ws_stride int16 (16-byte aligned): rows 0..7 = ws_stride records of
                     // 4 x int16 per direction (kNnRec; direction 0 first) = index of each query's NN per metric in the last
                     // iteration; rows 8..15 = ws_stride float4 of scratch (the balanced walk's minima per query)
  int ws_valid;      //   1: nn_ws holds the NNs of the iteration before this launch's first one
  int ws_stride;
  int pred_mode;     // diagnostics (houv_debug_set("solve_predict")): 0 normal; 1 always predict direction B (every A-win takes the
                     // repair path); 2 rescan everything (no skipping: the round-1 epilogue's work)
  unsigned long long* stats;   // houv_debug_set("solve_stats", device pointer): [0] sub-tile visits the lanes of the pruned sweeps
                               // asked for, [1] sub-tile steps their waves executed, [2] pruned wave-sweeps, [3] brute wave-sweeps,
                               // [4] shader clocks (s_memtime) and [5] 100-MHz ticks (s_memrealtime) summed over the workgroups'
                               // loops: [4]/[5] x 100 MHz = the clock the chip sustained under THIS kernel's load; pruned kernels:
                               // [6] Chamfer terms computed and [7] terms possible (2 x metrics), per workgroup-iteration
  unsigned long long* walk_hist;   // houv_debug_set("solve_walk_hist", device pointer): 16 counters, slot = the term mask `need` of a
                                   // pruned sweep, +1 per walking wave (the unit of stats[2]); read where it is used only (fresh)
  unsigned long long* cull_stats;  // houv_debug_set("solve_cull_stats", device pointer): 4 counters of the box tests' group cull
                                   // (prune_masks): groups tested, boxes surviving, per-query tests executed, per-query tests of a
                                   // loop over all boxes; read where it is used only (fresh)
  // Stage scheduling (houv_solve_stage[_pruned]).  sched_ws == nullptr: one workgroup per hypothesis, n_iters
  // iterations (houv_solve_iterate[_pruned]).  Otherwise a persistent grid draws tickets from sched_ws[0]: ticket t is the item
  // (chunk = t / ninst, hypothesis = t % ninst), chunk_iters iterations of the stage's n_iters (the last chunk what is left).
  int* sched_ws;     // int32 [4 + P*K]: [0] ticket counter, [1] status (non-zero: a poll ran out of time), [2..3] spare,
                     // [4 + h] = done[h], chunks of hypothesis h that are finished AND published; zeroed by the call
  int chunk_iters;
  unsigned long long* sched;   // houv_debug_set("solve_sched", device pointer): per XCD (HW_REG_XCC_ID, 0..7) 4 counters: items run
                               // by its workgroups, sum of the workgroups' durations, earliest start, latest end (100-MHz ticks
                               // of s_memrealtime; the caller presets the minima to all ones); read where it is used only (fresh)
};

constexpr int kRescanBatch = 4;       // references per batch of a rescan's LDS reads (recover_nn)
// pruned mode: every kRefresh-th iteration rescans every computed term and so refreshes its remembered NNs.  Same-device A/B of the
// balanced walk (profiles/r03_ab_refresh.txt): 1 -> 0.697, 2 -> 0.667, 4 -> 0.658, 6 -> 0.657, 8 -> 0.658 us per
// hypothesis-iteration, identical results; round 2's owner walk, whose steps cost more, preferred 2 (r02_ab_pruned_refresh.txt).
constexpr int kRefresh = 4;
// term masks: a term is dropped for at most this many iterations in a row, then computed once; 0: no limit (a launch's last
// iteration computes every term anyway).  A limit bounds how stale a dropped term's remembered NNs get -- its visit lists are long
// for the one iteration of its return -- but every forced return is a term computed for nothing.  Same-device A/B at 2,048 points
// (profiles/r11_ab_term_anchors.txt): no limit 0.3510 / 0.3520, 12 -> 0.3520 / 0.3526, 6 -> 0.3544 / 0.3550 us per
// hypothesis-iteration, identical results.
constexpr int kTermMaxAge = 0;
// stage scheduling: 100-MHz ticks (s_memrealtime) a poll of done[h] allows per iteration of the stage: 20 ms, derived where it is used
constexpr unsigned long long kPollTicksPerIter = 2000000ull;

// words of an item's scalars in LDS (solve_kernel's `iw`)
constexpr int kItemSteps = 0, kItemIters = 1, kItemWsValid = 2, kItemInst = 3, kItemClk = 4;   // [kItemClk .. +3]: the stats' two stamps

// the XCD (0..7) this wave runs on
__device__ __forceinline__ int xcc_id() {
  int v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v & 7;
}

struct Smem {
  float4* tgt;     // [Mpad]
  float4* mov;     // [Npad]
  double* state;   // [24]
  double* adam;    // [2][2] step size and sqrt(bias correction 2) of Adam: slot = step parity (see the scalar tail)
  float* pose;     // [kPoseFloats] the whole Pose of the current parameters: R row-major [0..8], T [9..11], backward intermediates
  float* acc;      // [8][kAccStride]   slot = metric*2 + dir
  float* red;      // [2 dirs][NW][kRedStride]
  unsigned* hist;  // [kHistSets][256]
  int* ctl;        // [8 + NW]
  float4* tbox;    // [2*64] lo/hi boxes of the target's 32-point sub-tiles   (pruned mode only); x, y, z only: the .w lanes
                   // [0..47] hold the term masks' stale record poses (R | T per metric), see kStalePose
  float4* mbox;    // [2*64] same for the moved cloud, rebuilt every iteration
  SortedStage st;  // staging of the balanced pruned sweep (pruned mode only)
  float* anchor;   // [kAnchorFloats] term masks (pruned mode only): the eight cd records, [kTermAges] the drop ages, | the source radius
};
// The term masks themselves travel in ctl[0]: bits 0..3 = terms needed over the target points (direction B), 4..7 = over the
// moved points (direction A); written by thread 0 in the scalar tail (and the prologue), read by every thread after barrier L6.
constexpr int kAnchorFloats = kTermAnchorFloats + 4;   // [kTermAnchorFloats] = radius of the source cloud about the origin
constexpr int kTermAges = 8;      // sm.anchor[kTermAges] as unsigned: 8 bits per metric, iterations in a row with a term dropped
// Records of the term masks (term_anchor_masks, houv_math.h).  A term computed in the iteration that just ended has that
// iteration's pose as its record pose: it is still in sm.pose when the rule runs.  At most one term per metric is older (it was
// dropped): its record pose, 12 floats per metric, lives in the .w lanes of sm.tbox -- tile_boxes writes .w = 0 there once per
// launch in the prologue, prune_masks uses x, y, z of a box only (its read-ahead loads the whole float4), and sm.tbox has 128
// entries whatever the cloud size.
constexpr int kStalePose = 4;     // floats between two consecutive entries of a stale pose (one float4 of sm.tbox each)


// prune: 0 brute force, 2 pruned (balanced walk: + staging for block * q queries)
// PRUNE == 3: the balanced walk over 64-point SUPER-tiles (pairs of sub-tiles) for clouds of 2049..4096 points: the clouds are
// padded to multiples of 64 points
__host__ __device__ inline int pad_unit(int prune) { return prune == 3 ? 2 * kSub : kSub; }

__host__ __device__ inline size_t smem_bytes(int N, int M, int block, int prune, int q) {
  const int pu = pad_unit(prune);
  int npad = (N + pu - 1) / pu * pu, mpad = (M + pu - 1) / pu * pu;
  if (prune) npad = mpad = (npad > mpad ? npad : mpad);   // the balanced walk parks a mask half in EITHER cloud's .w lanes
  const int nw = block / 64;
  const size_t nq = (size_t)block * q;
  return (size_t)(npad + mpad) * 16 + 28 * 8 + kPoseFloats * 4 + 8 * kAccStride * 4 + (size_t)2 * nw * kRedStride * 4 +
         kHistSets * kHistBins * 4 + (8 + nw) * 4 + 64 + (prune ? 2 * 128 * 16 + nq * 2 + 132 * 4 + kAnchorFloats * 4 : 0);
}

// nq = BLOCK * Q for the balanced pruned sweep (PRUNE != 0), 0 otherwise; pu = pad_unit(PRUNE)
__device__ inline Smem carve(unsigned char* base, int N, int M, int block, int nq, int pu) {
  int npad = (N + pu - 1) / pu * pu, mpad = (M + pu - 1) / pu * pu;
  if (nq) npad = mpad = (npad > mpad ? npad : mpad);
  const int nw = block / 64;
  Smem s;
  s.tgt = reinterpret_cast<float4*>(base);
  s.mov = s.tgt + mpad;
  s.state = reinterpret_cast<double*>(s.mov + npad);
  s.adam = s.state + 24;
  s.pose = reinterpret_cast<float*>(s.adam + 4);
  s.acc = s.pose + kPoseFloats;
  s.red = s.acc + 8 * kAccStride;
  s.hist = reinterpret_cast<unsigned*>(s.red + 2 * nw * kRedStride);
  s.ctl = reinterpret_cast<int*>(s.hist + kHistSets * kHistBins);
  // 16-byte alignment by OFFSET arithmetic on the shared segment (a pointer -> integer -> pointer round trip hides the LDS
  // address space from the compiler: the box reads of the pruned sweep became flat_load_dwordx3 + s_waitcnt vmcnt(0))
  const size_t box_off = ((size_t)(reinterpret_cast<unsigned char*>(s.ctl + 8 + nw) - base) + 15) & ~(size_t)15;
  s.tbox = reinterpret_cast<float4*>(base + box_off);
  s.mbox = s.tbox + 128;
  // balanced pruned sweep only (the pointers are never used otherwise)
  s.st.hist = reinterpret_cast<int*>(s.mbox + 128);
  s.st.order = reinterpret_cast<unsigned short*>(s.st.hist + 132);
  s.anchor = reinterpret_cast<float*>(s.st.order + nq);   // nq is even: 4-byte aligned
  return s;
}

// A uniform value made opaque to the optimiser where the iteration loop uses it: what the loop derives from it in VALU
// (conversions, quotients, LDS addresses) is recomputed there instead of being hoisted out of the loop into VGPRs that spilled.
template <typename T>
__device__ __forceinline__ T fresh(T v) {
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ const float* fresh_lds(const float* p) {
  typedef const float __attribute__((address_space(3))) * lds_f;
  return (const float*)(lds_f)(size_t)fresh((unsigned)(size_t)(lds_f)p);
}

// Exact selection of the `ksel` smallest of the BLOCK*Q register-resident keys (fp32 bit patterns of non-negative
// distances; 0xFFFFFFFF marks "not a point"): houv_solve.h's radix select.
// Ties at the threshold are taken in (thread, k) order -- torch.topk leaves tie order unspecified.
template <int BLOCK, int Q>
__device__ __forceinline__ void select_smallest(const unsigned (&key)[Q], int ksel, unsigned* hist, int* ctl,
                                                bool (&sel)[Q], int& hrot) {
  constexpr int NW = BLOCK / 64;
  const int tid = tid_x(), lane = tid & 63, wave = tid >> 6;
  RadixState rs{0u, 0u, ksel, 0};
#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    unsigned* h = radix_rotate<BLOCK>(hist, hrot, tid);
#pragma unroll
    for (int k = 0; k < Q; ++k) radix_count(h, key[k], pass, lane, rs);
    __syncthreads();
    radix_pick(h, pass, lane, rs);
  }
  const unsigned prefix = rs.prefix;
  const int remaining = rs.remaining, neq = rs.neq;
  if (neq == remaining) {
#pragma unroll
    for (int k = 0; k < Q; ++k) sel[k] = key[k] <= prefix;
  } else {
    int e = 0;
#pragma unroll
    for (int k = 0; k < Q; ++k) e += (key[k] == prefix) ? 1 : 0;
    const int incl = wave_incl_scan_dpp(e);
    __syncthreads();
    if (lane == 63) ctl[8 + wave] = incl;
    __syncthreads();
    int rank = incl - e;
    for (int w = 0; w < NW; ++w) rank += (w < wave) ? ctl[8 + w] : 0;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const bool eq = key[k] == prefix;
      sel[k] = key[k] < prefix || (eq && rank < remaining);
      rank += eq ? 1 : 0;
    }
  }
}

// ---- epilogue building blocks ------------------------------------------------------------------------------------
// Per metric and direction the scalar tail needs   S = sum sqrt(d)   over the selected queries, and -- for the ONE
// direction that wins the min of houv.py:212-221 -- G = sum c, GP = sum c p^T with c = mask * (moved - target) / sqrt(d),
// p = un-moved source point.  S needs only the distances the sweep already holds; G and GP need the identity of the
// nearest neighbour, i.e. the exact rescan of the winning sub-tile (32 references x ~11 instructions per query and
// metric: 3/4 of the epilogue's instruction count).  Since round 2 the rescans run only where the gradient flows.
//   DIR == 1 ("A"): queries are this lane's moved points (count = N), references the target cloud.
//   DIR == 0 ("B"): queries are this lane's target points (count = M), references the moved cloud.
constexpr int kGradN = 12;

// wave-level DPP sum; lane 63 parks the total
__device__ __forceinline__ void park(float v, float* dst) {
  v = wave_sum_to_lane63(v);
  if ((tid_x() & 63) == 63) *dst = v;
}

// selections of one direction: bit k of bits[m] = query k of this lane takes part in metric m's mean
template <int BLOCK, int Q, int NMET>
__device__ __forceinline__ void select_all(const Smem& sm, const float (&best)[Q][NMET], int count, int k_full, int k_view,
                                           unsigned need, int& hrot, unsigned (&bits)[NMET]) {
  bool valid[Q], sel[Q];
  unsigned key[Q];
#pragma unroll
  for (int m = 0; m < NMET; ++m) {
    // The drivers' view terms take all points (N == M, k_view == count: no select below), but houv_solve_iterate also accepts
    // N != M and k_view < count: the view terms then select like the full metric (tests/test_gpu_solve_select.py runs both).
    const int ksel = (m == 0) ? k_full : k_view;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      valid[k] = pt_index<BLOCK>(k) < count;
      key[k] = valid[k] ? __float_as_uint(best[k][m]) : 0xFFFFFFFFu;
      sel[k] = valid[k];
    }
    // an unneeded term's selection is never used; `need` is workgroup-uniform, so the barriers inside stay matched
    if (ksel < count && ((need >> m) & 1u)) select_smallest<BLOCK, Q>(key, ksel, sm.hist, sm.ctl, sel, hrot);
    unsigned b = 0u;
#pragma unroll
    for (int k = 0; k < Q; ++k) b |= sel[k] ? (1u << k) : 0u;
    bits[m] = b;
  }
}

// this lane's share of S for one metric (k order; no finite distance -> NaN like torch's min/topk/sqrt chain)
template <int Q>
__device__ __forceinline__ float lane_sqrt_sum(const float (&bd)[Q], unsigned selbits) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < Q; ++k)
    if ((selbits >> k) & 1u) s += (bd[k] < INFINITY) ? sqrtf(bd[k]) : NAN;
  return s;
}

// this lane's share of G[3], GP[9] for one metric: exact NN recovery + products, per query (nothing is kept per query)
// WS: remember each query's NN for the pruned search's next bounds (metric MET's int16 of the query's record at ws + ws_off)
template <int BLOCK, int Q, int MET, int DIR, bool WS>
__device__ __forceinline__ void lane_grad_sums(const Smem& sm, const float4* __restrict__ refs, const float (&qx)[Q],
                                               const float (&qy)[Q], const float (&qz)[Q], const float (&bd)[Q],
                                               const int (&bt)[Q], unsigned selbits, int count, const float (&px)[Q],
                                               const float (&py)[Q], const float (&pz)[Q], float (&g)[kGradN], buf_t ws,
                                               int ws_off) {
  const int rot = tid_x() & (kSub - 1);
#pragma unroll
  for (int i = 0; i < kGradN; ++i) g[i] = 0.f;
  float R[9], T[3];
  if constexpr (DIR == 0) load_rt(sm.pose, R, T);
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    int jn;
    const float4 nn = recover_nn<MET, kRescanBatch, true>(refs + bt[k] * kTrk, qx[k], qy[k], qz[k], bd[k], rot, jn);
    if (WS && pt_index<BLOCK>(k) < count)
      __builtin_amdgcn_raw_buffer_store_b16((unsigned short)(bt[k] * kTrk + jn), ws, tid_x() * kNnRec,
                                            ws_off + pt_base<BLOCK>(k) * kNnRec + MET * 2, 0);
    if ((selbits >> k) & 1u) {
      const float s = (bd[k] < INFINITY) ? sqrtf(bd[k]) : NAN;
      const float inv = 1.0f / s;   // d == 0 -> inf, and 0*inf = NaN below, as torch's sqrt backward gives
      float dx, dy, dz, sx, sy, sz;
      if constexpr (DIR == 1) {
        dx = qx[k] - nn.x; dy = qy[k] - nn.y; dz = qz[k] - nn.z;
        sx = px[k]; sy = py[k]; sz = pz[k];
      } else {
        dx = nn.x - qx[k]; dy = nn.y - qy[k]; dz = nn.z - qz[k];
        const float ux = nn.x - T[0], uy = nn.y - T[1], uz = nn.z - T[2];
        sx = R[0] * ux + R[3] * uy + R[6] * uz;   // R^T (p' - T)
        sy = R[1] * ux + R[4] * uy + R[7] * uz;
        sz = R[2] * ux + R[5] * uy + R[8] * uz;
      }
      if constexpr (MET == 1) dx = 0.f;
      if constexpr (MET == 2) dy = 0.f;
      if constexpr (MET == 3) dz = 0.f;
      const float cx = dx * inv, cy = dy * inv, cz = dz * inv;
      g[0] += cx; g[1] += cy; g[2] += cz;
      g[3] += cx * sx; g[4] += cx * sy; g[5] += cx * sz;
      g[6] += cy * sx; g[7] += cy * sy; g[8] += cy * sz;
      g[9] += cz * sx; g[10] += cz * sy; g[11] += cz * sz;
    }
  }
}

// S of every metric of one direction: per-lane sums -> wave totals parked in red[dir][wave][m*13]
template <int BLOCK, int Q, int NMET>
__device__ __forceinline__ void park_sqrt_sums(const float (&best)[Q][NMET], const unsigned (&selbits)[NMET], unsigned need,
                                               float* red_wave) {
  float bd[Q];
#pragma unroll
  for (int m = 0; m < NMET; ++m) {
    if (!((need >> m) & 1u)) continue;   // final_sums writes +inf for an unneeded term
#pragma unroll
    for (int k = 0; k < Q; ++k) bd[k] = best[k][m];
    park(lane_sqrt_sum<Q>(bd, selbits[m]), red_wave + m * kAccN);
  }
}

// G, GP of the metrics in `mask` of one direction -> red[dir][wave][m*13 + 1 ..]; no barrier in here
template <int BLOCK, int Q, int NMET, int DIR, bool WS>
__device__ __forceinline__ void park_grad_sums(const Smem& sm, const float4* __restrict__ refs, const float (&qx)[Q],
                                               const float (&qy)[Q], const float (&qz)[Q], const float (&best)[Q][NMET],
                                               const int (&btile)[Q][NMET], const unsigned (&selbits)[NMET], unsigned mask,
                                               int count, const float (&px)[Q], const float (&py)[Q], const float (&pz)[Q],
                                               float* red_wave, buf_t ws, int ws_off) {
  float bd[Q], g[kGradN];
  int bt[Q];
#define HOUV_GRAD(MET)                                                                                              \
  if ((mask >> MET) & 1u) {                                                                                         \
    _Pragma("unroll") for (int k = 0; k < Q; ++k) {                                                                 \
      bd[k] = best[k][MET];                                                                                         \
      bt[k] = btile[k][MET];                                                                                        \
    }                                                                                                               \
    lane_grad_sums<BLOCK, Q, MET, DIR, WS>(sm, refs, qx, qy, qz, bd, bt, selbits[MET], count, px, py, pz, g,        \
                                           ws, ws_off);                                                             \
    _Pragma("unroll") for (int i = 0; i < kGradN; ++i) park(g[i], red_wave + MET * kAccN + 1 + i);                  \
  }
  HOUV_GRAD(0)
  if constexpr (NMET == 4) {
    HOUV_GRAD(1)
    HOUV_GRAD(2)
    HOUV_GRAD(3)
  }
#undef HOUV_GRAD
}

// cross-wave sums (wave order) of the parked partials into sm.acc[(metric*2+dir)][..]; call after a barrier.
// S of a term that was not computed (bit clear in `need`) is +inf: picked_direction and solve_tail_loss then take the other
// direction, which the term mask proved to be the winner, with the bits the brute-force kernel gives it.
template <int BLOCK, int NMET>
__device__ __forceinline__ void final_sums(const Smem& sm, int dir, bool want_s, unsigned grad_mask, unsigned need) {
  constexpr int NW = BLOCK / 64;
  const int tid = tid_x();
  if (tid < NMET * kAccN) {
    const int m = tid / kAccN, i = tid % kAccN;
    if ((i == 0) ? want_s : (((grad_mask >> m) & 1u) != 0u)) {
      const float* r = sm.red + (size_t)dir * NW * kRedStride + tid;
      float a = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) a += r[w * kRedStride];
      if (i == 0 && !((need >> m) & 1u)) a = INFINITY;
      sm.acc[(m * 2 + dir) * kAccStride + i] = a;
    }
  }
}

// which direction wins each metric's min: bit m set = direction 1 (over the moved points).  The rule of the scalar tail
// (torch.min(cat([first, second])): first wins ties), evaluated by every thread on the same LDS values.
template <int NMET>
__device__ __forceinline__ unsigned picked_direction(const Smem& sm, int k_full, int k_view) {
  unsigned pick = 0u;
#pragma unroll
  for (int m = 0; m < NMET; ++m) {
    const float kk = (float)((m == 0) ? k_full : k_view);
    const float cd0 = sm.acc[(m * 2 + 0) * kAccStride] / kk, cd1 = sm.acc[(m * 2 + 1) * kAccStride] / kk;
    pick |= (cd0 <= cd1) ? 0u : (1u << m);
  }
  return pick;
}

// this lane's source point k (pt_index) of the pair's cloud `src` (N points): one buffer_load_dwordx3; 0 past the end
template <int BLOCK>
__device__ __forceinline__ void load_src_point(buf_t src, int k, int N, float& x, float& y, float& z) {
  x = y = z = 0.f;
  if (pt_index<BLOCK>(k) < N) {
    const auto v = __builtin_amdgcn_raw_buffer_load_b96(src, tid_x() * 12, pt_base<BLOCK>(k) * 12, 0);
    x = __uint_as_float(v[0]); y = __uint_as_float(v[1]); z = __uint_as_float(v[2]);
  }
}

// Mis-prediction repair (rare): metric MET's gradient flows through direction A, but A's rescans were skipped because the
// previous iteration's winner was B and A's sweep state is gone.  Redo A for this one metric: moved points, single-metric
// sweep (bit-identical minima and sub-tiles: same expression tree, same tie rule), selection, rescan, sums.
template <int BLOCK, int Q, int MET>
__device__ __forceinline__ void repair_direction_a(const Smem& sm, buf_t src, int N, int mpad, int k_sel,
                                                   int& hrot, float* red_wave) {
  float sx[Q], sy[Q], sz[Q], mx[Q], my[Q], mz[Q];
  float R[9], T[3];
  load_rt(sm.pose, R, T);
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    load_src_point<BLOCK>(src, k, N, sx[k], sy[k], sz[k]);
    move_point(R, T, sx[k], sy[k], sz[k], mx[k], my[k], mz[k]);
  }
  float bd[Q];
  int bt[Q];
  sweep_one<Q, MET>(sm.tgt, mpad / kTrk, mx, my, mz, bd, bt);
  bool sel[Q];
  unsigned key[Q], bits = 0u;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    sel[k] = pt_index<BLOCK>(k) < N;
    key[k] = sel[k] ? __float_as_uint(bd[k]) : 0xFFFFFFFFu;
  }
  if (k_sel < N) select_smallest<BLOCK, Q>(key, k_sel, sm.hist, sm.ctl, sel, hrot);
#pragma unroll
  for (int k = 0; k < Q; ++k) bits |= sel[k] ? (1u << k) : 0u;
  float g[kGradN];
  lane_grad_sums<BLOCK, Q, MET, 1, false>(sm, sm.tgt, mx, my, mz, bd, bt, bits, N, sx, sy, sz, g, src, 0);
#pragma unroll
  for (int i = 0; i < kGradN; ++i) park(g[i], red_wave + MET * kAccN + 1 + i);
}

// PRUNE: 0 the brute-force sweep; 2 / 3 the exact pruned search of houv_sweep.h (balanced walk over sub-tiles / super-tiles).
// Waves per SIMD the register budget is set for: 4 (128 VGPRs); 8 (64 VGPRs) where a lane owns one point.
template <int BLOCK, int Q, int NMET, int PRUNE>
__global__ __launch_bounds__(BLOCK, (Q == 1 ? 8 : 4)) void solve_kernel(SolveArgs a) {
  static_assert(PRUNE == 0 || PRUNE == 2 || PRUNE == 3, "brute force, or the balanced walk over sub-tiles / super-tiles");
  constexpr int TS = (PRUNE == 3) ? 1 : 0;                      // visit masks over super-tiles of 32 << TS references
  constexpr int kPad = kSub << TS;
  extern __shared__ __attribute__((aligned(512))) unsigned char smem_raw[];   // 512 B: the pruned walk's XOR-rotated gathers
  // Scheduling diagnostic: this workgroup's start stamp and item count wait in free ctl words (not in registers)
  if (fresh(a.sched) && tid_x() == 0) {
    int* ctl = carve(smem_raw, a.N, a.M, BLOCK, PRUNE ? BLOCK * Q : 0, kPad).ctl;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    ctl[2] = (int)(unsigned)t0;
    ctl[3] = (int)(unsigned)(t0 >> 32);
    ctl[4] = 0;
  }
  // The ticket loop of a stage (a.sched_ws set; one pass and no tickets otherwise).  Everything below it is one ITEM: what a
  // launch of houv_solve_iterate[_pruned] does for one hypothesis, with the item's own steps_done / n_iters / ws_valid.
#pragma unroll 1
  for (;;) {
  // The thread index is taken anew per item (and per use inside the iteration loop): what the prologue derives from it per lane
  // is computed in the item -- not once in front of the ticket loop, where it would stay in VGPRs through every iteration loop.
  // For the same reason the prologue's uniform values that the vector unit forms (the poll limit, the pose, Adam's scalars, the
  // padding vector) start from fresh() arguments.
  const int N = a.N, M = a.M;
  const Smem sm = carve(smem_raw, N, M, BLOCK, PRUNE ? BLOCK * Q : 0, kPad);
  const int tid = tid_x();
  const int ninst = a.P * a.K;
  int inst = blockIdx.x, steps_done = a.steps_done, n_iters = a.n_iters, ws_valid = a.ws_valid, chunk = 0;
  if (a.sched_ws) {
    // Tickets are drawn in order by resident workgroups, chunk-major: the earlier chunk of this hypothesis was drawn ninst
    // tickets before, so it is finished or running -- the wait below checks, it does not schedule, and cannot deadlock at any
    // grid size (the chain ends at chunk 0).
    if (tid == 0) {
      int t = atomicAdd(a.sched_ws, 1);
      const int c = t / ninst;
      if (t < sched_items(ninst, a.n_iters, a.chunk_iters) && c > 0) {
        // Consumer side of the hand-off (one lane polls relaxed, then ONE agent acquire; its wait holds the barrier below
        // until this CU's L1 is invalidated; plain loads follow).  The poll is bounded in TIME: the chain a wait depends on is
        // the earlier chunks of this one hypothesis, one after the other, i.e. fewer than n_iters iterations; the longest
        // iteration of a supported shape is the 4096-point brute-force kernel's, 2 x 4096^2 point pairs on one CU = 1.6 ms
        // (4 x the 0.78 ms a workgroup-iteration of profiles/r03_pmc_summary.txt's 2048-point brute-force launch takes, at one
        // workgroup per CU instead of two).  kPollTicksPerIter allows 20 ms per iteration: 12 x that, for a slow clock and for
        // other streams' kernels sharing the CU.
        const int* done = a.sched_ws + 4 + (t - c * ninst);
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        const unsigned long long limit = (unsigned long long)fresh(a.n_iters) * kPollTicksPerIter;   // (formed here, not hoisted)
        while (__hip_atomic_load(done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c) {
          if (__builtin_amdgcn_s_memrealtime() - t0 > limit) {
            __hip_atomic_store(a.sched_ws + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            t = 0x7fffffff;   // every thread leaves the ticket loop
            break;
          }
          __builtin_amdgcn_s_sleep(32);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      sm.ctl[1] = t;
    }
    __syncthreads();   // the ticket, and behind an acquire: the earlier chunk's state (must be fresh: plain loads behind this
                       // acquire, the guide's "plain stores + agent release / agent acquire + plain loads" form) and its NN
                       // records in nn_ws rows 0..7 (may be stale: any in-range remembered index is an attained bound, so a stale
                       // record costs visits, not correctness; rows 8..15 are scratch within an iteration)
    const int t = __builtin_amdgcn_readfirstlane(sm.ctl[1]);
    if (t >= sched_items(ninst, a.n_iters, a.chunk_iters)) break;
    chunk = t / ninst;
    inst = t - chunk * ninst;
    steps_done = a.steps_done + chunk * a.chunk_iters;
    n_iters = sched_item_iters(a.n_iters, a.chunk_iters, chunk);
    ws_valid = (a.ws_valid != 0 || chunk > 0) ? 1 : 0;
    if (fresh(a.sched) && tid == 0) sm.ctl[4] += 1;
  } else {
    // XCD-aware placement: workgroups b and b+8 share an XCD (and its L2), so give each XCD a contiguous
    // range of hypotheses -> the K restarts of one pair read the pair's clouds through ONE L2.
    if ((ninst & 7) == 0) inst = (blockIdx.x & 7) * (ninst >> 3) + (blockIdx.x >> 3);
    if (fresh(a.sched) && tid == 0) sm.ctl[4] = 1;
  }
  // The item's scalars wait in LDS, not in SGPRs, through the iteration loop (item(i) where a uniform value is needed, iw[i] in
  // the one-thread tails): the 64 bytes smem_bytes adds for alignment leave at least 52 behind the last array.
  int* const iw = PRUNE ? reinterpret_cast<int*>(sm.anchor + kAnchorFloats) : sm.ctl + 8 + BLOCK / 64;
  if (tid == 0) {
    iw[kItemSteps] = steps_done;
    iw[kItemIters] = n_iters;
    iw[kItemWsValid] = ws_valid;
    iw[kItemInst] = inst;
  }
  auto item = [&](int i) {
    return __builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(fresh_lds(reinterpret_cast<const float*>(iw + i))));
  };
  const int pair = inst / a.K;
  const buf_t src = make_buf(a.src + (size_t)pair * N * 3, N * 12);
  const float* __restrict__ tgt = a.tgt + (size_t)pair * M * 3;
  const int npad = (N + kPad - 1) / kPad * kPad, mpad = (M + kPad - 1) / kPad * kPad;
  // padding references never win; the +inf is opaque so that this vector is the prologue's own (as the same constant as the
  // walk's it was kept in four VGPRs from the head of the ticket loop on, and spilled)
  const float inf = __uint_as_float(fresh(0x7f800000u));
  const float4 pad4 = make_float4(inf, inf, inf, 0.f);

  for (int j = tid; j < mpad; j += BLOCK) sm.tgt[j] = (j < M) ? make_float4(tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2], 0.f) : pad4;
  for (int j = N + tid; j < npad; j += BLOCK) sm.mov[j] = pad4;
  if (tid < 24) sm.state[tid] = a.state[(size_t)inst * 24 + tid];
  for (int j = tid; j < kHistBins; j += BLOCK) sm.hist[j] = 0u;   // radix-select histogram set 0 (radix_rotate takes it from there)
  if constexpr (PRUNE) {
    if (tid < 132) sm.st.hist[tid] = 0;                           // list-length bins of the balanced pruned sweep
  }
  int hrot = 0;
  __syncthreads();
  // this hypothesis' workspace (pruned mode; brute force: src again, never accessed): byte offsets of the NN records of
  // direction 0 (NN of the target points in the moved cloud) and direction 1 (NN of the moved points in the target)
  buf_t ws = src;
  const int ws_b = 0, ws_a = a.ws_stride * kNnRec;
  float4* ws_res = nullptr;   // balanced walk: per-query minima on their way back to the owning lanes (rows 8..15)
  if constexpr (PRUNE) {
    ws = make_buf(a.nn_ws + (size_t)inst * 16 * a.ws_stride, 32 * a.ws_stride);
    ws_res = reinterpret_cast<float4*>(a.nn_ws + ((size_t)inst * 16 + 8) * a.ws_stride);
    float tx0[Q], ty0[Q], tz0[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const int i = pt_index<BLOCK>(k);
      const float4 v = (i < M) ? sm.tgt[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      tx0[k] = v.x; ty0[k] = v.y; tz0[k] = v.z;
    }
    tile_boxes<BLOCK, Q, TS>(tx0, ty0, tz0, M, mpad / kPad, sm.tbox);   // the target is static: boxes once per launch
  }
  // Adam's step-dependent scalars (two double pow()) are computed off the critical path: by thread kAdamTid (another wave,
  // hence another SIMD, when the workgroup has one) one iteration ahead, into the slot of the step's parity.
  constexpr int kAdamTid = BLOCK >= 128 ? 64 : 0;
  if (tid == 0) {
    float p[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = (float)sm.state[k];
    Pose f;
    pose_forward(p, fresh(a.angle_base), fresh(a.trans_mode), f);
    store_pose(sm.pose, f);
  }
  if (tid == kAdamTid) {
    const int step = steps_done + 1;
    const AdamScalars asc = adam_scalars(step, fresh(a.lr), fresh(a.beta1), fresh(a.beta2));
    sm.adam[(step & 1) * 2 + 0] = asc.step_size;
    sm.adam[(step & 1) * 2 + 1] = asc.bc2_sqrt;
  }
  if constexpr (PRUNE) {
    // term masks: the first iteration of a launch computes every term (the records do not travel through `state`); the
    // radius of the source cloud about the origin is one max-reduce (a NaN or Inf coordinate gives +inf: no term is ever dropped)
    float r2 = 0.f;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      float x, y, z;
      load_src_point<BLOCK>(src, k, N, x, y, z);
      const float v = __builtin_fmaf(z, z, __builtin_fmaf(y, y, x * x));
      r2 = (v <= r2) ? r2 : ((v < INFINITY) ? v : INFINITY);
    }
    r2 = wave_fmax_to_lane63(r2);   // r2 is never NaN; a maximum does not depend on the order it is taken in
    if ((tid & 63) == 63) sm.red[tid >> 6] = r2;
    if (tid == 0) {
      sm.ctl[0] = (int)(((1u << NMET) - 1u) * 0x11u);
      reinterpret_cast<unsigned*>(sm.anchor)[kTermAges] = 0u;
    }
  }
  __syncthreads();
  if constexpr (PRUNE) {
    if (tid == 0) {   // sm.red is next written after barrier L1, which this thread reaches after these reads
      float r2 = 0.f;
      for (int w = 0; w < BLOCK / 64; ++w) r2 = fmaxf(r2, sm.red[w]);
      sm.anchor[kTermAnchorFloats] = sqrtf(r2) * 1.000001f;   // rounded up
    }
  }

  if (a.stats && tid == 0) {   // two stamps per ITEM (not per iteration), only when the counters are on
    const unsigned long long clk0 = __builtin_amdgcn_s_memtime(), rt0 = __builtin_amdgcn_s_memrealtime();
    iw[kItemClk] = (int)(unsigned)clk0;
    iw[kItemClk + 1] = (int)(unsigned)(clk0 >> 32);
    iw[kItemClk + 2] = (int)(unsigned)rt0;
    iw[kItemClk + 3] = (int)(unsigned)(rt0 >> 32);
  }
  constexpr int NW = BLOCK / 64;
  constexpr unsigned kAllMet = (1u << NMET) - 1u;
  // Gradient-direction prediction: bit m = "metric m's min was won by direction A (over the moved points) in the previous
  // iteration".  A's rescans + G/GP sums run only for predicted-A metrics (A's sweep state is gone by the time the winner
  // is known); B's run exactly for the metrics B wins; a metric predicted B but won by A is repaired (rare).  Results do
  // not depend on the prediction.  The pruned kernel's bounds are distances to REMEMBERED nearest neighbours (nn_ws): any
  // remembered point gives a valid, attained bound, so a skipped rescan only leaves an older neighbour in place (a
  // slightly looser bound); every kRefresh-th iteration rescans every term it computes to keep them fresh.
  unsigned pred_a = kAllMet;
  // this wave's row of the reduction scratch of a direction, formed where it is used from the opaque thread index (formed here,
  // once, the two addresses lived in VGPRs through every walk of the loop)
  auto red_row = [&](int dir) { return sm.red + ((size_t)dir * NW + (tid_x() >> 6)) * kRedStride; };
#pragma unroll 1
  for (int it = 0; it < item(kItemIters); ++it) {
    if (a.pred_mode == 1) pred_a = 0u;
    const bool allgrad = a.pred_mode == 2 || ((PRUNE != 0) && (((item(kItemSteps) + it) % kRefresh) == 0 || (it == 0 && item(kItemWsValid) == 0)));
    // Term masks (term_anchor_masks, houv_math.h): a term that provably loses its metric's min is not computed -- no search, no
    // selection, no sums, no rescans; its remembered NNs stay as they are (an older neighbour is still an attained bound).  The
    // proof also settles the prediction: where B's term is dropped A is the winner, and the other way round.  Workgroup-uniform.
    unsigned need_a = kAllMet, need_b = kAllMet;
    if constexpr (PRUNE != 0) {
      const unsigned w = (unsigned)__builtin_amdgcn_readfirstlane(*reinterpret_cast<const int*>(fresh_lds(reinterpret_cast<const float*>(sm.ctl))));
      need_b = w & kAllMet;
      need_a = (w >> 4) & kAllMet;
    }
    const unsigned grad_a = (allgrad ? kAllMet : (pred_a | ~need_b)) & need_a;
    {
      // ---- move this lane's source points, publish them as references for sweep B ----
      float sx[Q], sy[Q], sz[Q], mx[Q], my[Q], mz[Q];
      float R[9], T[3];
      load_rt(fresh_lds(sm.pose), R, T);
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        const int i = pt_index<BLOCK>(k);
        const bool ok = i < N;
        load_src_point<BLOCK>(src, k, N, sx[k], sy[k], sz[k]);
        move_point(R, T, sx[k], sy[k], sz[k], mx[k], my[k], mz[k]);
        if (ok) sm.mov[i] = make_float4(mx[k], my[k], mz[k], 0.f);
      }
      __syncthreads();   // L1 -- writers: every thread's moved points (sm.mov); readers: the walk of sweep A (its queries), sweep B
      // ---- sweep A: moved -> target ----
      bool pruned_now = false;
      float best[Q][NMET];
      int btile[Q][NMET];
      if constexpr (PRUNE) {
        tile_boxes<BLOCK, Q, TS>(mx, my, mz, N, npad / kPad, sm.mbox);   // read by sweep B after the next barriers, and by sweep A's
                                                                         // group cull: each wave its own lanes' entries
        pruned_now = (it > 0) || (item(kItemWsValid) != 0);
      }
      if (need_a != 0u) {   // none of A's terms needed: no walk, no selection, no sums (the move and the boxes above are for sweep B)
        if (pruned_now) {
          if constexpr (PRUNE != 0)
            pruned_sweep_sorted<BLOCK, Q, NMET, TS>(sm.tgt, sm.tbox, mpad / kPad, sm.mbox, sm.mov, sm.tgt, sm.mov, mx, my, mz, ws, ws_a, N,
                                                need_a, sm.st, ws_res, best, btile, a.stats, fresh(a.walk_hist), fresh(a.cull_stats));
        } else {
          sweep<Q, NMET>(sm.tgt, mpad / kTrk, mx, my, mz, best, btile);
          if (a.stats && (tid_x() & 63) == 0) atomicAdd(&a.stats[3], 1ull);
        }
        // ---- epilogue A: selection, S of every needed metric, G/GP of the predicted-A metrics; one barrier ----
        unsigned sel[NMET];
        select_all<BLOCK, Q, NMET>(sm, best, N, a.k_full, a.k_view, need_a, hrot, sel);
        park_sqrt_sums<BLOCK, Q, NMET>(best, sel, need_a, red_row(1));
        park_grad_sums<BLOCK, Q, NMET, 1, PRUNE != 0>(sm, sm.tgt, mx, my, mz, best, btile, sel, grad_a, N, sx, sy, sz, red_row(1), ws,
                                                     ws_a);
      }
      __syncthreads();   // L2 -- writers: every wave's parked partials of direction A (red_row(1)); readers: wave 0's final_sums
      final_sums<BLOCK, NMET>(sm, 1, true, grad_a, need_a);
    }
    unsigned pick_a;
    {
      // ---- sweep B: target -> moved ----
      float tx[Q], ty[Q], tz[Q];
#pragma unroll
      for (int k = 0; k < Q; ++k) {
        const int i = pt_index<BLOCK>(k);
        const float4 v = (i < M) ? sm.tgt[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        tx[k] = v.x; ty[k] = v.y; tz[k] = v.z;
      }
      const bool pruned_now = (PRUNE != 0) && ((it > 0) || (item(kItemWsValid) != 0));
      // The barriers between B's S and B's G / GP: once with B's sweep state alive around them, once without (need_b is
      // workgroup-uniform, so all waves meet in the same pair).  Written twice so that B's minima are scoped to the branch that
      // computes them: as values merged after a skipped sweep they were carried around the iteration loop, in spilled VGPRs.
      auto pick_winners = [&]() {
        __syncthreads();   // L3 -- writers: every wave's parked S of direction B (red_row(0)); readers: wave 0's final_sums
        final_sums<BLOCK, NMET>(sm, 0, true, 0u, need_b);
        __syncthreads();   // L4 -- writers: wave 0's S of both directions (sm.acc; A's since L2); readers: every thread's picked_direction
        pick_a = picked_direction<NMET>(sm, fresh(a.k_full), fresh(a.k_view));
        return (allgrad ? kAllMet : (~pick_a & kAllMet)) & need_b;   // an unneeded term's +inf never wins
      };
      unsigned grad_b = 0u;
      if (need_b != 0u) {
        float best[Q][NMET];
        int btile[Q][NMET];
        if (pruned_now) {
          if constexpr (PRUNE != 0)
            pruned_sweep_sorted<BLOCK, Q, NMET, TS>(sm.mov, sm.mbox, npad / kPad, sm.tbox, sm.tgt, sm.tgt, sm.mov, tx, ty, tz, ws, ws_b, M,
                                                need_b, sm.st, ws_res, best, btile, a.stats, fresh(a.walk_hist), fresh(a.cull_stats));
        } else {
          sweep<Q, NMET>(sm.mov, npad / kTrk, tx, ty, tz, best, btile);
          if (a.stats && (tid_x() & 63) == 0) atomicAdd(&a.stats[3], 1ull);
        }
        // ---- epilogue B: selection and S first; then the winners are known to every thread ----
        unsigned sel[NMET];
        select_all<BLOCK, Q, NMET>(sm, best, M, a.k_full, a.k_view, need_b, hrot, sel);
        park_sqrt_sums<BLOCK, Q, NMET>(best, sel, need_b, red_row(0));
        grad_b = pick_winners();
        park_grad_sums<BLOCK, Q, NMET, 0, PRUNE != 0>(sm, sm.mov, tx, ty, tz, best, btile, sel, grad_b, M, tx, ty, tz, red_row(0), ws,
                                                     ws_b);
      } else {   // none of B's terms needed: every metric's winner is A, proven
        pick_winners();
      }
      // ---- repair: won by A, but A's rescans were skipped ----
      const unsigned miss = pick_a & ~grad_a & kAllMet;
      if (miss) {
        if (miss & 1u) repair_direction_a<BLOCK, Q, 0>(sm, src, N, mpad, a.k_full, hrot, red_row(1));
        if constexpr (NMET == 4) {
          if (miss & 2u) repair_direction_a<BLOCK, Q, 1>(sm, src, N, mpad, a.k_view, hrot, red_row(1));
          if (miss & 4u) repair_direction_a<BLOCK, Q, 2>(sm, src, N, mpad, a.k_view, hrot, red_row(1));
          if (miss & 8u) repair_direction_a<BLOCK, Q, 3>(sm, src, N, mpad, a.k_view, hrot, red_row(1));
        }
      }
      __syncthreads();   // L5 -- writers: every wave's parked G / GP of direction B and of the repairs; readers: wave 0's final_sums
      final_sums<BLOCK, NMET>(sm, 0, false, grad_b, kAllMet);
      if (miss) final_sums<BLOCK, NMET>(sm, 1, false, miss, kAllMet);
    }
    pred_a = pick_a;
    // No barrier here (there was one): every sm.acc entry the tail reads was written by final_sums, i.e. by threads below
    // NMET * kAccN <= 64 -- wave 0, the tail's own wave, whose LDS accesses complete in program order; sm.adam's slot of this step
    // was written before barrier L6 of the previous iteration (or in the prologue).
    static_assert(NMET * kAccN <= 64, "final_sums runs on the scalar tail's wave");
    __builtin_amdgcn_wave_barrier();

    // ---- per-hypothesis scalar tail: loss, closed-form gradient, Adam, next pose ----
    if (kAdamTid != 0 && tid_x() == kAdamTid && it + 1 < iw[kItemIters]) {   // next iteration's Adam scalars, while thread 0 works below
      const int step = iw[kItemSteps] + it + 2;
      const AdamScalars asc = adam_scalars(step, fresh(a.lr), fresh(a.beta1), fresh(a.beta2));
      sm.adam[(step & 1) * 2 + 0] = asc.step_size;
      sm.adam[(step & 1) * 2 + 1] = asc.bc2_sqrt;
    }
    if (tid_x() == 0) {
      const int k_full = fresh(a.k_full), k_view = fresh(a.k_view);
      const float loss_scale = fresh(a.loss_scale);
      const double lr = fresh(a.lr), beta1 = fresh(a.beta1), beta2 = fresh(a.beta2), eps = fresh(a.eps);
      const int angle_base = fresh(a.angle_base), trans_mode = fresh(a.trans_mode);
      Pose f;
      load_pose(f, sm.pose);        // the forward of the current parameters, kept from the end of the previous tail / the prologue
      TailLoss r;
      solve_tail_loss<NMET>(sm.acc, kAccStride, f, k_full, k_view, loss_scale, trans_mode, r);
      if (iw[kItemSteps] + it == fresh(a.steps_done) + fresh(a.n_iters) - 1)   // the stage's last iteration (a launch's: its own last)
        store_outputs(a.out_score, a.out_loss, a.out_R, a.out_T, a.out_grad, a.out_cd, iw[kItemInst], f, r);
      if constexpr (PRUNE != 0) {
        // every term computed in this iteration renews its record: its value here, its pose is this iteration's (sm.pose until
        // the store below); a dropped term's record stays as it is
#pragma unroll
        for (int m = 0; m < NMET; ++m) {
          if ((need_b >> m) & 1u) sm.anchor[2 * m] = r.cd[m][0];
          if ((need_a >> m) & 1u) sm.anchor[2 * m + 1] = r.cd[m][1];
        }
      }
      const int step = iw[kItemSteps] + it + 1;
      const AdamScalars asc{sm.adam[(step & 1) * 2 + 0], sm.adam[(step & 1) * 2 + 1]};
      solve_tail_step(r.g, sm.state, a.f64_params, asc, beta1, beta2, eps, angle_base, trans_mode, f);
      if constexpr (PRUNE != 0) {
        // The coming iteration's term masks.  Every term is computed on the first iteration of a launch (prologue), on the last
        // one (its eight cd are outputs) and always under pred_mode 2; in between term_anchor_masks drops what the records and the
        // pose just stepped to prove unnecessary (for at most kTermMaxAge iterations in a row where that is set).
        unsigned next = kAllMet | (kAllMet << 4), ages = 0u;
        const bool all_next = fresh(a.pred_mode) == 2 || it + 2 >= iw[kItemIters];
        if (!all_next) {
          const unsigned have = need_b | (need_a << 4);
          float* stale = reinterpret_cast<float*>(sm.tbox) + 3;
          next = term_anchor_masks<NMET>(sm.anchor, sm.pose, stale, kStalePose, ~have & 0xffu, f.R, f.T,
                                         sm.anchor[kTermAnchorFloats]);
          const unsigned old_ages = reinterpret_cast<const unsigned*>(sm.anchor)[kTermAges];
#pragma unroll
          for (int m = 0; m < NMET; ++m) {
            unsigned age = (old_ages >> (8 * m)) & 0xffu;
            age = (((next >> m) & (next >> (4 + m)) & 1u) != 0u) ? 0u : age + 1u;
            if (kTermMaxAge > 0 && age > (unsigned)kTermMaxAge) {
              next |= 0x11u << m;
              age = 0u;
            }
            if (age > 0xffu) age = 0xffu;
            ages |= age << (8 * m);
            // a term computed in this iteration and dropped in the coming one: this iteration's pose becomes its stale record pose
            if (((have & ~next) >> m) & 0x11u) {
#pragma unroll
              for (int i = 0; i < 12; ++i) stale[(m * 12 + i) * kStalePose] = sm.pose[i];
            }
          }
        }
        reinterpret_cast<unsigned*>(sm.anchor)[kTermAges] = ages;
        sm.ctl[0] = (int)next;
        if (a.stats) {
          atomicAdd(&a.stats[6], (unsigned long long)(__popc(need_a) + __popc(need_b)));
          atomicAdd(&a.stats[7], (unsigned long long)(2 * NMET));
        }
      }
      store_pose(sm.pose, f);
      if (kAdamTid == 0 && it + 1 < iw[kItemIters]) {                       // single-wave workgroups: no other wave to do it
        const AdamScalars nxt = adam_scalars(step + 1, lr, beta1, beta2);
        sm.adam[((step + 1) & 1) * 2 + 0] = nxt.step_size;
        sm.adam[((step + 1) & 1) * 2 + 1] = nxt.bc2_sqrt;
      }
    }
    // L6 -- writers: thread 0's next pose (sm.pose), term masks (sm.ctl[0]) and state, thread kAdamTid's Adam scalars; readers:
    // every thread's move of the next iteration.  It also ends this iteration's reads of sm.mov (rescans of direction B) before the next move overwrites it.
    __syncthreads();
  }
  if (tid_x() < 24) a.state[(size_t)item(kItemInst) * 24 + tid_x()] = sm.state[tid_x()];   // (the prologue's address is not kept alive)
  if (a.stats && tid_x() == 0) {
    const unsigned long long clk0 = (unsigned long long)(unsigned)iw[kItemClk] | ((unsigned long long)(unsigned)iw[kItemClk + 1] << 32);
    const unsigned long long rt0 = (unsigned long long)(unsigned)iw[kItemClk + 2] | ((unsigned long long)(unsigned)iw[kItemClk + 3] << 32);
    atomicAdd(&a.stats[4], __builtin_amdgcn_s_memtime() - clk0);
    atomicAdd(&a.stats[5], __builtin_amdgcn_s_memrealtime() - rt0);
  }
  if (!fresh(a.sched_ws)) break;
  // Producer side of the hand-off: plain stores (state above, the NN records in the epilogues) -> every storing wave waits for
  // its stores -> workgroup barrier -> one lane: agent release, wait, relaxed agent store of done[h].  The barrier is also the
  // one between this item's last LDS access and the next item's prologue.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid_x() == 0) {
    const int t = sm.ctl[1], c = t / ninst;   // this item's ticket is still there: the next one is drawn below this
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(a.sched_ws + 4 + (t - c * ninst), c + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  }
  if (fresh(a.sched) && tid_x() == 0) {
    unsigned long long* s = fresh(a.sched) + 4 * xcc_id();
    const int* ctl = carve(smem_raw, a.N, a.M, BLOCK, PRUNE ? BLOCK * Q : 0, kPad).ctl;
    const unsigned long long t0 = (unsigned long long)(unsigned)ctl[2] | ((unsigned long long)(unsigned)ctl[3] << 32);
    const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
    atomicAdd(s + 0, (unsigned long long)ctl[4]);
    atomicAdd(s + 1, t1 - t0);
    atomicMin(s + 2, t0);
    atomicMax(s + 3, t1);
  }
}

// Workgroups of a stage's persistent grid: what the chip holds at once (never more than there are hypotheses);
// houv_debug_set("solve_max_workgroups") caps it for the tests.
template <typename Kernel>
int stage_grid(Kernel kernel, const SolveArgs& a, int block, size_t bytes, const char* who) {
  int dev = 0, cus = 0, per_cu = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, bytes);
  if (e != hipSuccess || cus < 1 || per_cu < 1) {
    set_error("%s: cannot size the persistent grid (%d CUs x %d workgroups): %s", who, cus, per_cu, hipGetErrorString(e));
    return 0;
  }
  long long grid = (long long)cus * per_cu;
  if (grid > (long long)a.P * a.K) grid = (long long)a.P * a.K;
  const int cap = g_debug.max_workgroups.load();
  if (cap > 0 && grid > cap) grid = cap;
  // every workgroup draws one ticket past the last item
  if (sched_items64(a.P * a.K, a.n_iters, a.chunk_iters) + grid > 0x7fffffffLL) {
    set_error("%s: too many (hypothesis, chunk) items for one stage", who);
    return 0;
  }
  return (int)grid;
}

template <typename Kernel>
int launch_kernel(Kernel kernel, const SolveArgs& a, int block, size_t bytes, hipStream_t s, const char* who) {
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) { set_error("%s: cannot reserve %zu B of LDS: %s", who, bytes, hipGetErrorString(e)); return 0; }
  int grid = a.P * a.K;
  if (a.sched_ws) {
    grid = stage_grid(kernel, a, block, bytes, who);
    if (grid < 1) return 0;
    e = hipMemsetAsync(a.sched_ws, 0, (4 + (size_t)a.P * a.K) * sizeof(int), s);
    if (e != hipSuccess) { set_error("%s: cannot zero sched_ws: %s", who, hipGetErrorString(e)); return 0; }
  }
  kernel<<<grid, block, bytes, s>>>(a);
  return check_launch(who) ? 1 : 0;
}

template <int BLOCK, int Q, int PRUNE>
int launch(const SolveArgs& a, int use_views, hipStream_t s, const char* who) {
  const size_t bytes = smem_bytes(a.N, a.M, BLOCK, PRUNE, Q);
  if (use_views) return launch_kernel(solve_kernel<BLOCK, Q, 4, PRUNE>, a, BLOCK, bytes, s, who);
  return launch_kernel(solve_kernel<BLOCK, Q, 1, PRUNE>, a, BLOCK, bytes, s, who);
}

}  // namespace
}  // namespace houv

// The variant table: which solve_kernel<BLOCK, Q> serves clouds of max(N, M) points -- the SAME (BLOCK, Q) for the brute-force
// sweep and for the pruned search, so that both sum in the same order and agree bit for bit.  Q = 3 points per lane covers
// the sizes between the powers of two without idle lanes (768, 1536, 3072).  The pruned search (balanced walk,
// pruned_sweep_sorted) serves 257..2048 points with one visit-mask bit per 32-point sub-tile (PRUNE = 2) and 2049..4096 points with
// one bit per 64-point super-tile (PRUNE = 3; one 1024-thread workgroup per CU there, like the brute-force kernel).  tests/test_host_logic.py enumerates this table and fails when a variant
// has no size that the GPU tests compare with the CPU oracle.
extern "C" int houv_solve_variant(int N, int M, int pruned, int* block, int* points_per_lane, int* prune_mode) {
  using namespace houv;
  const int mx = N > M ? N : M;
  if (N <= 0 || M <= 0) {
    set_error("houv_solve_variant: bad cloud sizes N=%d M=%d", N, M);
    return 0;
  }
  if (mx > 4096) {
    set_error("houv_solve_iterate: clouds larger than 4096 points do not fit in 160 KiB of LDS (N=%d M=%d)", N, M);
    return 0;
  }
  // Small clouds: no idle waves (every wave of a workgroup runs the whole epilogue, points or not).  Measured and NOT kept
  // (profiles/r03_sizes.txt): one wave with 2 points per lane at 65..128 points (+7 %, but it regroups the sums, and the
  // statistical G14 rung is calibrated on this grouping), one wave with 3-4 points per lane up to 256 points and two waves up to
  // 512 points (5-6 % SLOWER than 4 waves with 1-2 points per lane).
  int b, q;
  if (mx <= 64) { b = 64; q = 1; }
  else if (mx <= 128) { b = 128; q = 1; }
  else if (mx <= 256) { b = 256; q = 1; }
  else if (mx <= 512) { b = 256; q = 2; }
  else if (mx <= 768) { b = 256; q = 3; }
  else if (mx <= 1024) { b = 256; q = 4; }
  else if (mx <= 1536) { b = 512; q = 3; }
  else if (mx <= 2048) { b = 512; q = 4; }
  else if (mx <= 3072) { b = 1024; q = 3; }
  else { b = 1024; q = 4; }
  if (block) *block = b;
  if (points_per_lane) *points_per_lane = q;
  // Up to 256 points (8 sub-tiles or fewer, one point per lane) the pruned search is not built: houv_solve_iterate_pruned then runs
  // the brute-force kernel -- the same result.  With Morton-ordered sub-tiles it did not pay up to 512 points either; with k-d leaves
  // it does from 257 on (profiles/r03_sizes.txt: 512 points 0.119 -> 0.093 us, 320 points 0.084 -> 0.071).  solver.PRUNED_MIN_POINTS
  // is the same bound.
  constexpr int kPrunedMinPoints = 257;
  if (prune_mode) *prune_mode = (!pruned || mx < kPrunedMinPoints) ? 0 : (mx > 2048) ? 3 : 2;
  return 1;
}

extern "C" int houv_solve_walk_variant(int need) {
  if (need < 0 || need > 15) {
    houv::set_error("houv_solve_walk_variant: the term mask of a direction is 0..15, got %d", need);
    return -1;
  }
  return (int)houv::walk_variant((unsigned)need);
}

extern "C" long long houv_solve_lds_bytes(int N, int M, int pruned) {
  using namespace houv;
  int block = 0, q = 0, mode = 0;
  if (!houv_solve_variant(N, M, pruned, &block, &q, &mode)) return -1;
  return (long long)smem_bytes(N, M, block, mode, q);
}

int houv::solve_check_args(const char* who, const SolveCommon& a, int use_views) {
  const int P = a.P, N = a.N, M = a.M;
  if (P < 0 || N <= 0 || M <= 0 || a.K <= 0 || a.n_iters <= 0 || a.steps_done < 0 || a.angle_base < 0 || a.angle_base > 3 ||
      a.trans_mode < 0 || a.trans_mode > 1) {
    set_error("%s: bad argument P=%d N=%d M=%d K=%d n_iters=%d steps_done=%d base=%d trans_mode=%d", who, P, N, M, a.K,
              a.n_iters, a.steps_done, a.angle_base, a.trans_mode);
    return 0;
  }
  if (P == 0) return 1;
  if (!a.src || !a.tgt || !a.state) {
    set_error("%s: null pointer", who);
    return 0;
  }
  // topk(k) over a direction with fewer than k points raises in the reference (model_utils_completion.py:91-92)
  const int kv = use_views ? a.k_view : 1;
  if (a.k_full < 1 || a.k_full > N || a.k_full > M || kv < 1 || kv > N || kv > M) {
    set_error("%s: top-k size out of range (k_full=%d k_view=%d N=%d M=%d)", who, a.k_full, a.k_view, N, M);
    return 0;
  }
  if ((long long)P * a.K > 0x7fffffffLL) {
    set_error("%s: too many hypotheses", who);
    return 0;
  }
  return 2;
}

// stage: houv_solve_stage[_pruned] (chunk_iters and sched_ws are looked at); otherwise one workgroup per hypothesis
static int solve_dispatch(const houv::SolveCommon& c, int use_views, short* nn_ws, int ws_valid, int ws_stride, bool prune,
                          void* stream, const char* who, bool stage = false, int chunk_iters = 0, int32_t* sched_ws = nullptr) {
  using namespace houv;
  const int ok = solve_check_args(who, c, use_views);
  if (ok < 2) return ok;
  if (stage && chunk_iters < 1) {
    set_error("%s: chunk_iters must be >= 1, got %d", who, chunk_iters);
    return 0;
  }
  if (stage && (!sched_ws || ((uintptr_t)sched_ws & 3))) {
    set_error("%s: sched_ws must be a 4-byte aligned int32 [4 + P*K] on the device", who);
    return 0;
  }
  const int N = c.N, M = c.M;
  // pred_mode / stats are diagnostics set through houv_debug_set(), never through the environment.
  SolveArgs a{c, nn_ws, ws_valid, ws_stride, g_debug.pred_mode.load(),
              reinterpret_cast<unsigned long long*>(g_debug.stats.load()),
              reinterpret_cast<unsigned long long*>(g_debug.walk_hist.load()),
              reinterpret_cast<unsigned long long*>(g_debug.cull_stats.load()),
              stage ? sched_ws : nullptr, stage ? chunk_iters : 0,
              reinterpret_cast<unsigned long long*>(g_debug.sched.load())};
  hipStream_t s = (hipStream_t)stream;
  const int mx = N > M ? N : M;
  int block = 0, q = 0, mode = 0;
  if (!houv_solve_variant(N, M, prune ? 1 : 0, &block, &q, &mode)) return 0;
  if (prune && (!nn_ws || ws_stride < mx || (ws_stride & 7))) {
    set_error("%s: pruned mode needs a workspace of 16 x ws_stride int16 per hypothesis, ws_stride >= max(N,M) and a multiple of 8", who);
    return 0;
  }
  // the kernel reads a query's NN record as one 8-byte load and its minima record as one 16-byte load
  if (prune && ((uintptr_t)nn_ws & 15)) {
    set_error("%s: the pruned-mode workspace must be 16-byte aligned", who);
    return 0;
  }
  if (prune && ws_valid < 0) {   // test aid: the pruned entry point with the search switched off = the brute-force kernel of this size
    a.ws_valid = 0;
    mode = 0;
  }
  if (mode == 0) a.nn_ws = nullptr;
  // one instantiation per row of the variant table (houv_solve_variant), x {views, no views}, x {brute force, pruned}
#define HOUV_GO(B_, Q_)                                                          \
  if (block == B_ && q == Q_) {                                                  \
    if (mode == 2) return launch<B_, Q_, ((B_ >= 256 && Q_ >= 2) ? 2 : 0)>(a, use_views, s, who);    \
    return launch<B_, Q_, 0>(a, use_views, s, who);                                   \
  }
  if (mx <= 2048) {
    HOUV_GO(64, 1) HOUV_GO(128, 1) HOUV_GO(256, 1) HOUV_GO(256, 2) HOUV_GO(256, 3) HOUV_GO(256, 4)
    HOUV_GO(512, 3) HOUV_GO(512, 4)
  } else {
    if (block == 1024 && q == 3) return mode == 3 ? launch<1024, 3, 3>(a, use_views, s, who) : launch<1024, 3, 0>(a, use_views, s, who);
    if (block == 1024 && q == 4) return mode == 3 ? launch<1024, 4, 3>(a, use_views, s, who) : launch<1024, 4, 0>(a, use_views, s, who);
  }
#undef HOUV_GO
  set_error("%s: no kernel variant <%d,%d>", who, block, q);
  return 0;
}

extern "C" int houv_solve_iterate(const float* src, const float* tgt, int P, int N, int M, int K, double* state,
                                  int steps_done, int n_iters, int angle_base, int trans_mode, int use_views,
                                  int f64_params, int k_full, int k_view, double lr, double beta1, double beta2,
                                  double eps, float loss_scale, float* out_score, float* out_loss, float* out_R,
                                  float* out_T, float* out_grad, float* out_cd, void* stream) {
  const houv::SolveCommon a{src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view,
                            lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd};
  return solve_dispatch(a, use_views, nullptr, 0, 0, false, stream, "houv_solve_iterate");
}

extern "C" int houv_solve_iterate_pruned(const float* src, const float* tgt, int P, int N, int M, int K, double* state,
                                         int steps_done, int n_iters, int angle_base, int trans_mode, int use_views,
                                         int f64_params, int k_full, int k_view, double lr, double beta1, double beta2,
                                         double eps, float loss_scale, float* out_score, float* out_loss, float* out_R,
                                         float* out_T, float* out_grad, float* out_cd, int16_t* nn_ws, int ws_valid,
                                         int ws_stride, void* stream) {
  const houv::SolveCommon a{src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view,
                            lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd};
  return solve_dispatch(a, use_views, (short*)nn_ws, ws_valid, ws_stride, true, stream, "houv_solve_iterate_pruned");
}

extern "C" int houv_solve_stage(const float* src, const float* tgt, int P, int N, int M, int K, double* state, int steps_done,
                                int n_iters, int angle_base, int trans_mode, int use_views, int f64_params, int k_full,
                                int k_view, double lr, double beta1, double beta2, double eps, float loss_scale,
                                float* out_score, float* out_loss, float* out_R, float* out_T, float* out_grad, float* out_cd,
                                int chunk_iters, int32_t* sched_ws, void* stream) {
  const houv::SolveCommon a{src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view,
                            lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd};
  return solve_dispatch(a, use_views, nullptr, 0, 0, false, stream, "houv_solve_stage", true, chunk_iters, sched_ws);
}

extern "C" int houv_solve_stage_pruned(const float* src, const float* tgt, int P, int N, int M, int K, double* state,
                                       int steps_done, int n_iters, int angle_base, int trans_mode, int use_views,
                                       int f64_params, int k_full, int k_view, double lr, double beta1, double beta2,
                                       double eps, float loss_scale, float* out_score, float* out_loss, float* out_R,
                                       float* out_T, float* out_grad, float* out_cd, int16_t* nn_ws, int ws_valid,
                                       int ws_stride, int chunk_iters, int32_t* sched_ws, void* stream) {
  const houv::SolveCommon a{src, tgt, P, N, M, K, state, steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view,
                            lr, beta1, beta2, eps, loss_scale, out_score, out_loss, out_R, out_T, out_grad, out_cd};
  return solve_dispatch(a, use_views, (short*)nn_ws, ws_valid, ws_stride, true, stream, "houv_solve_stage_pruned", true,
                        chunk_iters, sched_ws);
}
