// gemm.hip -- fp32 MFMA GEMM with fused epilogue for the DCP head (BASELINE configs[4]).
//
// The DCP feature head (registration/models/dcp.py:269-381) is GEMM-shaped: 1x1 convolutions of the DGCNN
// (:272-276), the Transformer's linear layers / attention products (:26-32, :198-243) and the soft-correspondence
// scores (:345-346).  The reference computes in fp32, and so does this kernel: v_mfma_f32_32x32x2_f32 is an exact
// k-ordered fmaf chain at the fp32 vector rate (157 TFLOP/s peak), so parity with the reference needs no mixed
// precision argument.
//
//   C[m,n] = epilogue( alpha * sum_k A[m,k] * Bop[k,n] )        batched over blockIdx.z = (zo, zi)
//   BT = true : B is [N,K] row-major (nn.Linear / conv weight [out,in], K^T of attention) -> C = A B^T
//   BT = false: B is [K,N] row-major (P V of attention)                                  -> C = A B
//   epilogue  : v = alpha*acc; v = v*scale[n] + shift[n] (eval BatchNorm folded) | v += shift[n] (bias);
//               v += residual[m,n]; v = max(v,0)
// Tile 128 x BN x 32, 512 threads = 8 waves (4x2), each wave a 32 x BN/2 block of 32x32 MFMA tiles; LDS tiles are
// stored k-major so an MFMA operand fetch is a conflict-free ds_read_b32 (lanes 0-31: 32 consecutive rows at k,
// lanes 32-63: the same rows at k+1); the next k-tile is prefetched into registers while the current one is
// multiplied.
#include <cstdlib>
#include "../../include/houv_hip.h"
#include "houv_common.h"
#include "houv_split.h"

namespace houv {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct GemmArgs {
  const float* A; const float* B; float* C;
  int M, N, K, lda, ldb, ldc;
  int inner;                                   // blockIdx.z = zo * inner + zi
  long long sAo, sAi, sBo, sBi, sCo, sCi;      // element strides of the two batch levels
  float alpha;
  const float* scale; const float* shift;      // per output column n (may be null)
  const float* residual; int ldr; long long sRo, sRi;
  int relu;
};

constexpr int BM = 128, BK = 32;

__device__ __forceinline__ float4 load4_guarded(const float* __restrict__ p, int valid, bool vec_ok) {
  // up to 4 consecutive floats starting at p; `valid` of them exist (0..4)
  if (vec_ok && valid >= 4) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (valid > 0) v.x = p[0];
  if (valid > 1) v.y = p[1];
  if (valid > 2) v.z = p[2];
  if (valid > 3) v.w = p[3];
  return v;
}

// 512-thread workgroups (8 waves, 80 registers, up to 6 waves per SIMD): against the removed 256-thread form (4 waves, 139-172
// registers) short-K shapes gain 15-25 % (conv 64->128: 47 -> 56, Q K^T: 73 -> 90 TFLOP/s) and the long-K ones are unchanged.
// GUARD = false: every tile is full and 16-byte aligned (M % 128 == 0, N % BN == 0, K % 32 == 0, leading dimensions and batch
// strides multiples of 4 floats -- checked by the launcher): the fetch is four plain global_load_dwordx4 per thread.  The guarded
// form costs more than its bounds checks suggest: its per-lane branches compile into ~130 instructions of exec-mask juggling
// between the second barrier and the MFMA loop of every k-tile (measured: 101.6 -> 117 TFLOP/s at 65536 x 512 x 512 without it).
template <int BN, bool BT, bool GUARD>
__global__ __launch_bounds__(512, 6) void gemm_f32_kernel(GemmArgs g) {
  constexpr int NWM = 4;                               // waves along M
  constexpr int NT = NWM * 128;                        // threads
  constexpr int MI = BM / (32 * NWM);                  // 32-row MFMA tiles per wave along M
  constexpr int LDA = BM + 1;                         // k-major tiles, +1 breaks the transposing writes' conflicts
  constexpr int LDB = BT ? (BN + 1) : (BN + 4);       // the [K,N] form is written with 16-byte stores
  constexpr int NI = BN / 64;                         // 32-wide MFMA tiles per wave along N
  constexpr int AREG = BM * BK / 4 / NT;              // float4 per thread per A tile
  constexpr int BREG = BN * BK / 4 / NT;
  constexpr int QK = BK / 4;                          // k-quads per row
  constexpr int RPI = NT / QK;                        // rows covered per pass
  __shared__ float As[BK * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[BK * LDB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int zo = blockIdx.z / g.inner, zi = blockIdx.z - zo * g.inner;
  const float* __restrict__ A = g.A + zo * g.sAo + zi * g.sAi;
  const float* __restrict__ B = g.B + zo * g.sBo + zi * g.sBi;
  float* __restrict__ C = g.C + zo * g.sCo + zi * g.sCi;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
  const bool vecA = ((g.lda & 3) == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0);
  const bool vecB = ((g.ldb & 3) == 0) && ((reinterpret_cast<uintptr_t>(B) & 15) == 0);

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[AREG], rb[BREG];
  auto fetch = [&](int k0) {
    // A tile: 128 rows x BK k; thread t -> row t/QK + RPI i, k-quad (t%QK)*4
#pragma unroll
    for (int i = 0; i < AREG; ++i) {
      const int row = m0 + tid / QK + RPI * i, k = k0 + (tid % QK) * 4;
      if constexpr (!GUARD) ra[i] = *reinterpret_cast<const float4*>(A + (size_t)row * g.lda + k);
      else ra[i] = (row < g.M) ? load4_guarded(A + (size_t)row * g.lda + k, g.K - k, vecA) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if constexpr (BT) {   // B[n][k]: same pattern as A
#pragma unroll
      for (int i = 0; i < BREG; ++i) {
        const int col = n0 + tid / QK + RPI * i, k = k0 + (tid % QK) * 4;
        if constexpr (!GUARD) rb[i] = *reinterpret_cast<const float4*>(B + (size_t)col * g.ldb + k);
        else rb[i] = (col < g.N) ? load4_guarded(B + (size_t)col * g.ldb + k, g.K - k, vecB) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    } else {              // B[k][n]: BK k-rows x BN cols; thread t -> k = t / (BN/4) + (256/(BN/4)) i, n-quad
      constexpr int QPR = BN / 4, RPP = NT / QPR;
#pragma unroll
      for (int i = 0; i < BREG; ++i) {
        const int k = k0 + tid / QPR + RPP * i, col = n0 + (tid % QPR) * 4;
        if constexpr (!GUARD) rb[i] = *reinterpret_cast<const float4*>(B + (size_t)k * g.ldb + col);
        else rb[i] = (k < g.K) ? load4_guarded(B + (size_t)k * g.ldb + col, g.N - col, vecB) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < AREG; ++i) {
      const int r = tid / QK + RPI * i, k = (tid % QK) * 4;
      As[(k + 0) * LDA + r] = ra[i].x; As[(k + 1) * LDA + r] = ra[i].y;
      As[(k + 2) * LDA + r] = ra[i].z; As[(k + 3) * LDA + r] = ra[i].w;
    }
    if constexpr (BT) {
#pragma unroll
      for (int i = 0; i < BREG; ++i) {
        const int c = tid / QK + RPI * i, k = (tid % QK) * 4;
        Bs[(k + 0) * LDB + c] = rb[i].x; Bs[(k + 1) * LDB + c] = rb[i].y;
        Bs[(k + 2) * LDB + c] = rb[i].z; Bs[(k + 3) * LDB + c] = rb[i].w;
      }
    } else {
      constexpr int QPR = BN / 4, RPP = NT / QPR;
#pragma unroll
      for (int i = 0; i < BREG; ++i) {
        const int k = tid / QPR + RPP * i, c = (tid % QPR) * 4;
        *reinterpret_cast<float4*>(&Bs[k * LDB + c]) = rb[i];
      }
    }
  };

  fetch(0);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
    __syncthreads();          // previous tile fully consumed
    stage();
    __syncthreads();
    if (k0 + BK < g.K) fetch(k0 + BK);     // prefetch the next tile into registers under the MFMAs
    const int kh = lane >> 5, rl = lane & 31;
    // operand fragments are double buffered in registers: the ds_reads of k-step s+1 are issued before the MFMAs of
    // k-step s, so their latency hides under 4 x 64 MFMA cycles even when all waves of a SIMD run in lock-step
    float a[2][MI], b[2][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i) a[0][i] = As[kh * LDA + wm * (32 * MI) + i * 32 + rl];
#pragma unroll
    for (int j = 0; j < NI; ++j) b[0][j] = Bs[kh * LDB + wn * (BN / 2) + j * 32 + rl];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      const int cur = (kk >> 1) & 1, nxt = cur ^ 1;
      if (kk + 2 < BK) {
#pragma unroll
        for (int i = 0; i < MI; ++i) a[nxt][i] = As[(kk + 2 + kh) * LDA + wm * (32 * MI) + i * 32 + rl];
#pragma unroll
        for (int j = 0; j < NI; ++j) b[nxt][j] = Bs[(kk + 2 + kh) * LDB + wn * (BN / 2) + j * 32 + rl];
      }
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
      // pin the schedule hipcc would otherwise undo (it sinks the next step's LDS reads below these MFMAs and then waits
      // for them with the matrix pipe idle): first the DS reads of step s+1, then the MFMAs of step s
      __builtin_amdgcn_sched_group_barrier(0x100, MI + NI, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, MI * NI, 0);
    }
  }

  // epilogue: C/D map of the 32x32 tile: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const float* __restrict__ Rsd = g.residual ? g.residual + zo * g.sRo + zi * g.sRi : nullptr;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
    if (GUARD && col >= g.N) continue;
    const float sc = g.scale ? g.scale[col] : 1.0f;
    const float sh = g.shift ? g.shift[col] : 0.0f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * (32 * MI) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (GUARD && row >= g.M) continue;
        float v = acc[i][j][r] * g.alpha;
        v = v * sc + sh;
        if (Rsd) v += Rsd[(size_t)row * g.ldr + col];
        if (g.relu) v = fmaxf(v, 0.f);
        C[(size_t)row * g.ldc + col] = v;
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------------------------
// fp32 GEMM on the bf16 matrix pipe: every operand element is split into three bf16 parts, x = hi + mid + lo (round-to-nearest
// at each step, so the parts carry 8 + 8 + 8 significant bits and the residuals are exact in fp32), and the product is
// accumulated in fp32 from the part products whose weight is >= 2^-16 of the leading one:
//   NPROD = 6:  hi*hi + hi*mid + mid*hi + hi*lo + mid*mid + lo*hi     (dropped terms <= 2^-24 relative: the size of an fp32 rounding)
//   NPROD = 3:  hi*hi + hi*mid + mid*hi                               (<= 2^-16 relative: 32x finer than TF32)
// bf16 x bf16 is exact in fp32 and v_mfma_f32_32x32x16_bf16 accumulates in fp32, so NPROD = 6 is an fp32 GEMM to within a small
// multiple of the fp32 MFMA kernel's own rounding error (test_gemm_on_the_bf16_pipe_is_fp32_grade in tests/test_gpu_dcp.py and the
// gemm tests of tests/test_gpu_dcp_ops.py measure both against fp64 on the same operands).  The matrix pipe
// runs bf16 at 16x the fp32-input rate (MI355X_MICROARCH.md, Matrix cores), so six products cost 6/16 of the fp32 MFMA time.
// A tile's elements are split ONCE, while it is staged into LDS (5.5 VALU instructions per element, in the MFMAs' shadow):
// three bf16 planes per operand, rows of 32 k padded to 80 bytes so that the 16 lanes of a ds_read_b128 group (16 rows) hit 16
// distinct 16-byte slots; an MFMA operand fragment (8 consecutive k of one row) is one ds_read_b128 per plane.
// Full, 16-byte aligned tiles and B given as [N,K] (every DCP linear / 1x1 convolution / score product); anything else runs
// the fp32-input kernel above.  Inf in an operand yields NaN (Inf - Inf in the residual), where the fp32 kernel yields Inf.
// ---------------------------------------------------------------------------------------------------------------
template <int BN, int NPROD>
__global__ __launch_bounds__(512, 2) void gemm_split_kernel(GemmArgs g) {
  static_assert(NPROD == 6 || NPROD == 3, "six products (fp32-grade) or three (2^-16)");
  constexpr int NPART = NPROD == 6 ? 3 : 2;
  constexpr int NT = 512, NWM = 4;
  constexpr int MI = BM / (32 * NWM);                  // 1
  constexpr int NI = BN / 64;                          // 32-wide MFMA tiles per wave along N
  constexpr int ROWB = 80;                             // bytes per LDS row: 32 bf16 + 16 B of padding
  constexpr int QK = BK / 4, RPI = NT / QK;            // 8 k-quads per row, 64 rows per pass
  constexpr int AREG = BM * BK / 4 / NT, BREG = BN * BK / 4 / NT;
  __shared__ __attribute__((aligned(16))) unsigned char As[NPART][BM * ROWB];
  __shared__ __attribute__((aligned(16))) unsigned char Bs[NPART][BN * ROWB];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int zo = blockIdx.z / g.inner, zi = blockIdx.z - zo * g.inner;
  const float* __restrict__ A = g.A + zo * g.sAo + zi * g.sAi;
  const float* __restrict__ B = g.B + zo * g.sBo + zi * g.sBi;
  float* __restrict__ C = g.C + zo * g.sCo + zi * g.sCi;
  const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;

  f32x16 acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 ra[AREG], rb[BREG];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < AREG; ++i)
      ra[i] = *reinterpret_cast<const float4*>(A + (size_t)(m0 + tid / QK + RPI * i) * g.lda + k0 + (tid % QK) * 4);
#pragma unroll
    for (int i = 0; i < BREG; ++i)
      rb[i] = *reinterpret_cast<const float4*>(B + (size_t)(n0 + tid / QK + RPI * i) * g.ldb + k0 + (tid % QK) * 4);
  };
  auto stage = [&]() {
#pragma unroll
    for (int i = 0; i < AREG; ++i) {
      uint2 parts[NPART];
      split4<NPART>(ra[i], parts);
      const int off = (tid / QK + RPI * i) * ROWB + (tid % QK) * 8;
#pragma unroll
      for (int p = 0; p < NPART; ++p) *reinterpret_cast<uint2*>(&As[p][off]) = parts[p];
    }
#pragma unroll
    for (int i = 0; i < BREG; ++i) {
      uint2 parts[NPART];
      split4<NPART>(rb[i], parts);
      const int off = (tid / QK + RPI * i) * ROWB + (tid % QK) * 8;
#pragma unroll
      for (int p = 0; p < NPART; ++p) *reinterpret_cast<uint2*>(&Bs[p][off]) = parts[p];
    }
  };

  const int kh = lane >> 5, rl = lane & 31;
  fetch(0);
  for (int k0 = 0; k0 < g.K; k0 += BK) {
    __syncthreads();          // previous tile fully consumed
    stage();
    __syncthreads();
    if (k0 + BK < g.K) fetch(k0 + BK);     // the next tile travels while this one is multiplied
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8 a[MI][NPART], b[NI][NPART];
#pragma unroll
      for (int p = 0; p < NPART; ++p) {
#pragma unroll
        for (int i = 0; i < MI; ++i)
          a[i][p] = *reinterpret_cast<const bf16x8*>(&As[p][(wm * (32 * MI) + i * 32 + rl) * ROWB + s * 32 + kh * 16]);
#pragma unroll
        for (int j = 0; j < NI; ++j)
          b[j][p] = *reinterpret_cast<const bf16x8*>(&Bs[p][(wn * (BN / 2) + j * 32 + rl) * ROWB + s * 32 + kh * 16]);
      }
      // smallest terms first; (pa, pb) = part indices of A and B
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          if constexpr (NPROD == 6) {
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][2], b[j][0], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][2], acc[i][j], 0, 0, 0);
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][1], acc[i][j], 0, 0, 0);
          }
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][0], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][1], acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
        }
    }
  }

  const float* __restrict__ Rsd = g.residual ? g.residual + zo * g.sRo + zi * g.sRi : nullptr;
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = n0 + wn * (BN / 2) + j * 32 + (lane & 31);
    const float sc = g.scale ? g.scale[col] : 1.0f;
    const float sh = g.shift ? g.shift[col] : 0.0f;
#pragma unroll
    for (int i = 0; i < MI; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * (32 * MI) + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        float v = acc[i][j][r] * g.alpha;
        v = v * sc + sh;
        if (Rsd) v += Rsd[(size_t)row * g.ldr + col];
        if (g.relu) v = fmaxf(v, 0.f);
        C[(size_t)row * g.ldc + col] = v;
      }
    }
  }
}

}  // namespace
}  // namespace houv

// Public op-level entry (used by houv_dcp_forward and by the tests).  trans_b: 1 -> B is [N,K] row-major (C = A B^T),
// 0 -> B is [K,N] row-major (C = A B).  batch = outer*inner problems; element strides per level.
extern "C" int houv_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                             int trans_b, int outer, int inner, long long sAo, long long sAi, long long sBo,
                             long long sBi, long long sCo, long long sCi, float alpha, const float* scale_or_null,
                             const float* shift_or_null, const float* residual_or_null, int ldr, long long sRo,
                             long long sRi, int relu, void* stream) {
  using namespace houv;
  if (M <= 0 || N <= 0 || K <= 0 || outer <= 0 || inner <= 0 || !A || !B || !C || lda < K || ldc < N ||
      (trans_b ? ldb < K : ldb < N) || (long long)outer * inner > 65535) {
    set_error("houv_gemm_f32: bad argument M=%d N=%d K=%d lda=%d ldb=%d ldc=%d batch=%dx%d", M, N, K, lda, ldb, ldc,
              outer, inner);
    return 0;
  }
  GemmArgs g{A, B, C, M, N, K, lda, ldb, ldc, inner, sAo, sAi, sBo, sBi, sCo, sCi, alpha, scale_or_null, shift_or_null,
             residual_or_null, ldr, sRo, sRi, relu};
  hipStream_t s = (hipStream_t)stream;
  const bool narrow = N <= 64;
  dim3 grid((N + (narrow ? 64 : 128) - 1) / (narrow ? 64 : 128), (M + BM - 1) / BM, outer * inner);
  // full, aligned tiles everywhere (every DCP shape at 2048 points): the unguarded kernels
  const int bn = narrow ? 64 : 128;
  const bool aligned16 = !((reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B)) & 15) &&
                         !((lda | ldb | (int)(sAo & 3) | (int)(sAi & 3) | (int)(sBo & 3) | (int)(sBi & 3)) & 3);
  const bool full = aligned16 && M % BM == 0 && N % bn == 0 && K % BK == 0;
  const int split = g_debug.gemm_split.load();               // 0: fp32-input MFMA; 6 / 3: bf16 part products (see gemm_split_kernel)
  if (split && full && trans_b) {
    if (narrow) { if (split == 6) gemm_split_kernel<64, 6><<<grid, 512, 0, s>>>(g); else gemm_split_kernel<64, 3><<<grid, 512, 0, s>>>(g); }
    else { if (split == 6) gemm_split_kernel<128, 6><<<grid, 512, 0, s>>>(g); else gemm_split_kernel<128, 3><<<grid, 512, 0, s>>>(g); }
    return check_launch("houv_gemm_f32") ? 1 : 0;
  }
  if (narrow) {
    if (trans_b) { if (full) gemm_f32_kernel<64, true, false><<<grid, 512, 0, s>>>(g); else gemm_f32_kernel<64, true, true><<<grid, 512, 0, s>>>(g); }
    else { if (full) gemm_f32_kernel<64, false, false><<<grid, 512, 0, s>>>(g); else gemm_f32_kernel<64, false, true><<<grid, 512, 0, s>>>(g); }
  } else {
    if (trans_b) { if (full) gemm_f32_kernel<128, true, false><<<grid, 512, 0, s>>>(g); else gemm_f32_kernel<128, true, true><<<grid, 512, 0, s>>>(g); }
    else { if (full) gemm_f32_kernel<128, false, false><<<grid, 512, 0, s>>>(g); else gemm_f32_kernel<128, false, true><<<grid, 512, 0, s>>>(g); }
  }
  return check_launch("houv_gemm_f32") ? 1 : 0;
}
