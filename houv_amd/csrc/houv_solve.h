// houv_solve.h -- what the two fused-loop kernels share: solve_kernel (solve.hip, clouds resident in LDS) and
// solve_large_kernel (solve_large.hip, clouds streamed).  The scalar tail they both run is solve_tail_loss / solve_tail_step in houv_math.h.
#pragma once
#include <stddef.h>

#include "houv_sweep.h"

namespace houv {

// The arguments of every solve entry point (include/houv_hip.h), as the entry points receive them and the kernels read them;
// checked on the host by solve_check_args (houv_common.h).
struct SolveCommon {
  const float* src;
  const float* tgt;
  int P, N, M, K;
  double* state;
  int steps_done, n_iters, angle_base, trans_mode, f64_params, k_full, k_view;
  double lr, beta1, beta2, eps;
  float loss_scale;
  float* out_score;
  float* out_loss;
  float* out_R;
  float* out_T;
  float* out_grad;
  float* out_cd;
};

constexpr int kRedStride = 4 * kAccN;   // per-wave partial sums of one direction: [metric][13]
constexpr int kHistBins = 256;          // 8-bit radix digits
constexpr int kHistSets = 3;            // rotating histograms: one barrier per radix pass (see radix_rotate)
constexpr int kPoseFloats = 28;         // sizeof(Pose) / 4 rounded up
static_assert(sizeof(Pose) <= kPoseFloats * 4 && offsetof(Pose, T) == 36, "pose[0..11] in LDS must be R | T");

__device__ __forceinline__ void store_pose(float* dst, const Pose& f) {
  const float* src = reinterpret_cast<const float*>(&f);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(Pose) / 4); ++i) dst[i] = src[i];
}
__device__ __forceinline__ void load_pose(Pose& f, const float* src) {
  float* dst = reinterpret_cast<float*>(&f);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(Pose) / 4); ++i) dst[i] = src[i];
}
__device__ __forceinline__ void load_rt(const float* pose, float (&R)[9], float (&T)[3]) {
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = pose[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) T[i] = pose[9 + i];
}

// src @ R^T + T (houv.py:102).  THE expression tree of a moved point: both kernels' searches, rescans and sums see these bits.
__device__ __forceinline__ void move_point(const float (&R)[9], const float (&T)[3], float sx, float sy, float sz, float& mx,
                                           float& my, float& mz) {
  mx = __builtin_fmaf(sz, R[2], __builtin_fmaf(sy, R[1], sx * R[0])) + T[0];
  my = __builtin_fmaf(sz, R[5], __builtin_fmaf(sy, R[4], sx * R[3])) + T[1];
  mz = __builtin_fmaf(sz, R[8], __builtin_fmaf(sy, R[7], sx * R[6])) + T[2];
}

// outputs of the LAST forward (houv.py:134-136: the final step is never observed); f = the pose the loss was taken at.
// The pointers come by value: through a reference to the kernel's argument block, solve_kernel<512, 3, 4, 2> spilled two more
// SGPRs.
__device__ __forceinline__ void store_outputs(float* out_score, float* out_loss, float* out_R, float* out_T, float* out_grad,
                                              float* out_cd, int inst, const Pose& f, const TailLoss& r) {
  if (out_score) out_score[inst] = r.score;
  if (out_loss) out_loss[inst] = r.loss;
  if (out_R)
    for (int k = 0; k < 9; ++k) out_R[(size_t)inst * 9 + k] = f.R[k];
  if (out_T)
    for (int k = 0; k < 3; ++k) out_T[(size_t)inst * 3 + k] = f.T[k];
  if (out_grad)
    for (int k = 0; k < 8; ++k) out_grad[(size_t)inst * 8 + k] = r.g[k];
  if (out_cd)
    for (int m = 0; m < 4; ++m)
      for (int d = 0; d < 2; ++d) out_cd[(size_t)inst * 8 + m * 2 + d] = r.cd[m][d];
}

// ---- exact 4-pass 8-bit radix select on LDS histograms ---------------------------------------------------------------
// The `ksel`-th smallest of a workgroup's keys (fp32 bit patterns of non-negative distances; 0xFFFFFFFF marks "not a point").
// A pass is   h = radix_rotate();  radix_count(h, key, ...) for every key of this thread;  __syncthreads();  radix_pick(h, ...).
//   * ONE barrier per pass: three histograms rotate (`hrot` = the one this pass fills, all-zero on entry).  While pass p
//     fills set hrot, every thread also clears set hrot+1, whose last readers (pass p-2) are all past the barrier of
//     pass p-1; after the barrier EVERY wave scans the 256 bins itself (one ds_read_b128 per lane + a DPP prefix sum),
//     so no broadcast through LDS and no second barrier is needed.
//   * pass 0 (sign + 7 exponent bits) sees a handful of distinct digits: plain LDS atomics would serialise 64 lanes
//     on one address, so the wave counts each digit with a ballot and ONE lane adds the count.
// After the four passes prefix = the ksel-th smallest key, neq = how many keys equal it, remaining = how many of those are
// still to be taken; how ties are taken is the caller's business.
struct RadixState {
  unsigned prefix, mask;
  int remaining, neq;
};

template <int BLOCK>
__device__ __forceinline__ unsigned* radix_rotate(unsigned* hist, int& hrot, int tid) {
  unsigned* h = hist + hrot * kHistBins;
  hrot = (hrot == kHistSets - 1) ? 0 : hrot + 1;
  for (int i = tid; i < kHistBins; i += BLOCK) hist[hrot * kHistBins + i] = 0u;
  return h;
}

// every lane of the wave calls this together (pass 0 ballots)
__device__ __forceinline__ void radix_count(unsigned* h, unsigned key, int pass, int lane, const RadixState& s) {
  if (pass == 0) {
    const unsigned digit = key >> 24;
    unsigned long long todo = __ballot(1);
    while (todo) {                                           // wave-uniform loop over the distinct digits
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);
      const unsigned long long m = __ballot(digit == d);
      if (lane == leader) atomicAdd(&h[d], (unsigned)__popcll(m));
      todo &= ~m;
    }
  } else if ((key & s.mask) == s.prefix) {
    atomicAdd(&h[(key >> (24 - 8 * pass)) & 255u], 1u);
  }
}

__device__ __forceinline__ void radix_pick(const unsigned* h, int pass, int lane, RadixState& s) {
  const int shift = 24 - 8 * pass;
  const uint4 hv = *reinterpret_cast<const uint4*>(h + 4 * lane);
  const int hh[4] = {(int)hv.x, (int)hv.y, (int)hv.z, (int)hv.w};
  const int tot = hh[0] + hh[1] + hh[2] + hh[3];
  int c = wave_incl_scan_dpp(tot) - tot;
  int fbin = 0, fc = 0, fn = 0;
  bool found = false;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const bool hit = c < s.remaining && s.remaining <= c + hh[b];
    fbin = hit ? 4 * lane + b : fbin;
    fc = hit ? c : fc;
    fn = hit ? hh[b] : fn;
    found = found || hit;
    c += hh[b];
  }
  const int src_lane = __ffsll((long long)__ballot(found)) - 1;   // exactly one lane holds the bin (1 <= remaining <= total)
  const int bin = __builtin_amdgcn_readlane(fbin, src_lane);
  s.prefix |= (unsigned)bin << shift;
  s.mask |= 255u << shift;
  s.remaining -= __builtin_amdgcn_readlane(fc, src_lane);
  s.neq = __builtin_amdgcn_readlane(fn, src_lane);
}

}  // namespace houv
