// houv_common.h -- shared device helpers + host error plumbing for libhouv_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <atomic>

#include "houv_math.h"

namespace houv {

constexpr int kWave = 64;     // CDNA wavefront
constexpr int kSub = 32;      // reference points per sub-tile: padding unit, bounding boxes and visit masks of the pruned search
constexpr int kTrk = 16;      // reference points per arg-min TRACKING unit (half a sub-tile): what `btile` counts and a rescan re-reads

// ---- host side ---------------------------------------------------------------------------------
void set_error(const char* fmt, ...);
// The argument checks every solve entry point shares, in one order (defined in solve.hip; SolveCommon: houv_solve.h).  Returns 0
// with the error set, 1 when there is nothing to do (P == 0), 2 when `a` may be launched.  Internal: not part of the C ABI.
struct SolveCommon;
__attribute__((visibility("hidden"))) int solve_check_args(const char* who, const SolveCommon& a, int use_views);
// The index step of the ordered scatter (defined in pointops_group.hip): a stable counting sort of keys[B][M] (each in [0, N)) by
// destination, giving the CSR inverse offsets[B][N+1], order[B][M] with the sources of a destination in ascending m.  A key
// outside [0, N) is skipped, or with `clamp` taken as the nearest of 0 and N-1.  Internal.
__attribute__((visibility("hidden"))) bool scatter_index_launch(const int* keys, int B, int N, int M, int* offsets, int* order,
                                                                hipStream_t stream, bool clamp = false);
inline bool check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return false;
  }
  return true;
}

// Diagnostic switches (houv_debug_set; tests, A/B scripts and bench.py only -- never the environment).  Results are proven
// independent of every switch except the two that select the matrix-pipe kernels (gemm_split, attn_split).
//   "solve_predict"   0 normal; 1 always predict direction B (every A-win takes the repair path); 2 rescan everything
//   "solve_stats"     device address of 8 uint64 counters the fused loop adds to (0 = off): see SolveArgs::stats
//   "solve_walk_hist" device address of 16 uint64 counters (0 = off): the term masks the pruned walks see, see SolveArgs::walk_hist
//   "solve_cull_stats" device address of 4 uint64 counters (0 = off): the group cull of the box tests, see SolveArgs::cull_stats
//   "solve_sched"     device address of 8 x 4 uint64 counters (0 = off): per XCD, what its workgroups ran and when, see SolveArgs::sched
//   "solve_max_workgroups"  houv_solve_stage: cap of the persistent grid (0 = off); a test aid, like ws_valid < 0
//   "knn_split"       houv_knn: 1 references split over the four waves of a workgroup (same lists), 0 the single-scan kernel
//   "attn_split"      houv_attention_f32: 1 bf16 matrix pipe with three-part splits (full tiles), 0 fp32-input MFMA kernel
//   "gemm_split"      houv_gemm_f32: 0 fp32-input MFMA, 6 / 3 = bf16 part products per fp32 product (gemm.hip, gemm_split_kernel)
struct DebugKnobs {
  std::atomic<int> pred_mode{0};
  std::atomic<unsigned long long> stats{0ull};
  std::atomic<unsigned long long> walk_hist{0ull};
  std::atomic<unsigned long long> cull_stats{0ull};
  std::atomic<unsigned long long> sched{0ull};
  std::atomic<int> max_workgroups{0};
  std::atomic<int> knn_split{1};         // houv_knn (N >= 512, k = 16 / 20): four waves per 64 queries, a quarter of the references each; 0: one wave per 64 queries
  std::atomic<int> attn_split{1};        // houv_attention_f32 on the bf16 matrix pipe (attention.hip, attention_split_kernel); 0: fp32-input MFMA
  std::atomic<int> gemm_split{6};        // houv_gemm_f32 on the bf16 matrix pipe: 6 / 3 part products per fp32 product (0: fp32-input MFMA)
};
extern DebugKnobs g_debug;

// ---- device side -------------------------------------------------------------------------------
// The four squared distances share dx,dy,dz.  MET 0: full 3-D; MET 1/2/3: coordinate x/y/z dropped
// (loss_view, registration/model_utils_completion.py:157-166).  The expression trees are fixed
// (explicit fma, compiled with -ffp-contract=off) so that the sweep and the index-recovery rescan
// produce bit-identical values.  MET 0 equals fma(dz,dz,fma(dy,dy,dx*dx)), the contraction nvcc
// applies to the reference's x2*x2+y2*y2+z2*z2 (chamfer3D.cu:33-36).
template <int MET>
__device__ __forceinline__ float metric_sqdist(float dx, float dy, float dz) {
  if constexpr (MET == 0) return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
  else if constexpr (MET == 1) return __builtin_fmaf(dz, dz, dy * dy);
  else if constexpr (MET == 2) return __builtin_fmaf(dz, dz, dx * dx);
  else return __builtin_fmaf(dy, dy, dx * dx);
}

__device__ __forceinline__ float min3f(float a, float b, float c) {
  return __builtin_fminf(__builtin_fminf(a, b), c);   // -> v_min3_f32
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// ---- DPP cross-lane helpers: pure VALU (v_*_dpp), no LDS crossbar round trip like __shfl's ds_bpermute_b32 ------
// dpp_ctrl encodings (GCN3+/CDNA): row_shr:n = 0x110+n, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ float dpp_f(float v) {   // masked-out / out-of-row lanes read 0
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, BANK_MASK, true));
}
template <int CTRL, int ROW_MASK = 0xf, int BANK_MASK = 0xf>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, BANK_MASK, true);
}

// Sum over the 64 lanes; the total is valid in LANE 63 ONLY (other lanes hold partial sums).  6 VALU instructions.
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
  v += dpp_f<0x111>(v);               // row_shr:1
  v += dpp_f<0x112>(v);               // row_shr:2
  v += dpp_f<0x114>(v);               // row_shr:4
  v += dpp_f<0x118>(v);               // row_shr:8   -> lane 15 of every row of 16 holds the row sum
  v += dpp_f<0x142, 0xa>(v);          // row_bcast:15 into rows 1 and 3
  v += dpp_f<0x143, 0xc>(v);          // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave sum
  return v;
}

// Maximum of NON-NEGATIVE ints over the 64 lanes, valid in LANE 63 ONLY (masked-out DPP sources read 0).
__device__ __forceinline__ int wave_max_to_lane63(int v) {
  v = max(v, dpp_i<0x111>(v));
  v = max(v, dpp_i<0x112>(v));
  v = max(v, dpp_i<0x114>(v));
  v = max(v, dpp_i<0x118>(v));
  v = max(v, dpp_i<0x142, 0xa>(v));
  v = max(v, dpp_i<0x143, 0xc>(v));
  return v;
}

// Maximum of floats over the 64 lanes, NaN left out (all NaN: NaN), valid in LANE 63 ONLY.  Any sign: a masked-out or
// out-of-row DPP source reads the lane's own value, not 0.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float fmax_dpp(float v) {
  return __builtin_fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xf, false)));
}
__device__ __forceinline__ float wave_fmax_to_lane63(float v) {
  v = fmax_dpp<0x111>(v);
  v = fmax_dpp<0x112>(v);
  v = fmax_dpp<0x114>(v);
  v = fmax_dpp<0x118>(v);
  v = fmax_dpp<0x142, 0xa>(v);
  v = fmax_dpp<0x143, 0xc>(v);
  return v;
}

// inclusive prefix sum across the 64 lanes, DPP form (7 VALU instructions)
__device__ __forceinline__ int wave_incl_scan_dpp(int x) {
  int v = x + dpp_i<0x111>(x);
  v += dpp_i<0x112>(x);
  v += dpp_i<0x113>(x);               // v[i] = x[i-3..i] within the row
  v += dpp_i<0x114, 0xf, 0xe>(v);     // row_shr:4 into lanes 4..15 of each row
  v += dpp_i<0x118, 0xf, 0xc>(v);     // row_shr:8 into lanes 8..15
  v += dpp_i<0x142, 0xa>(v);          // previous row's total into rows 1 and 3
  v += dpp_i<0x143, 0xc>(v);          // lane 31's total into rows 2 and 3
  return v;
}

// inclusive prefix sum across the 64 lanes of a wave
__device__ __forceinline__ int wave_incl_scan_i(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    int n = __shfl_up(v, o, kWave);
    if (lane >= o) v += n;
  }
  return v;
}

}  // namespace houv
