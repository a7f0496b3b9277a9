// pcn.hip -- the two device pieces of the PCN completion network (registration/models/pcn.py):
//
//   houv_mlp2_max   one PointNet block: a two-layer pointwise MLP whose channel-wise maximum over the points of a cloud is the
//                   epilogue of the second GEMM.  A workgroup owns 64 points of one cloud.  The hidden layer is produced 128
//                   channels at a time (GEMM 1 -> shift + ReLU -> LDS) and consumed at once as the k-slice of GEMM 2, whose
//                   64 x Cout accumulators stay in registers for the whole workgroup: the [B, N, H] activations never exist in
//                   memory and the [B, N, Cout] ones only when the caller asks for them.  Per-tile maxima go to a workspace and a
//                   second, tiny kernel folds them in tile order (one tile: straight to `pooled`).
//   houv_pcn_fold   the folding stage of PCN_decoder.forward (:108-125): the 5-wide per-point part of the first convolution in
//                   the vector ALU (the global feature's share arrives as one 512-vector per cloud), the 512 x 512 layer on the
//                   matrix pipe with the same k-slice scheme, and the 512 -> 3 layer as a fixed-order reduction of the
//                   accumulators.  Nothing wider than 3 channels per fine point reaches memory.
//
// Products run on v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation, an ordered fma chain over k.  No atomics, no
// allocation, every reduction in a fixed order: results are bit-identical from call to call.
#include <algorithm>

#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kT = HOUV_PCN_ROW_TILE;            // points per workgroup: two 32-row MFMA tiles
constexpr int kNT = 512;                         // 8 waves
constexpr int kHK = 128;                         // hidden channels per k-slice of the second layer
constexpr int kLDH = kT + 1;                     // k-major LDS tiles of 64 rows: the 32 lanes of a transposing write hit 32 banks
constexpr int kBK2 = 16;                         // k per staged tile of the second layer's weights
static_assert(kT == 64, "the wave layout below is written for two 32-row tiles");

// C/D layout of a 32x32 MFMA tile: column = lane & 31, row = acc_row(reg, lane)
__device__ __forceinline__ int acc_row(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// acc[i][j] += Hs[64 rows x kHK] . W[:, kbase .. kbase + kHK)^T.  Hs is k-major ([k][kLDH]); W is [COUT, ldw] row-major in
// global memory (LDG floats per row) and streams through Ws in tiles of kBK2, the next tile travelling in registers under the MFMAs of this one.
// Wave w owns the 32 * NI columns from w * 32 * NI on, for all 64 rows.  Starts and ends with a workgroup barrier.
template <int COUT, int LDG>
__device__ __forceinline__ void second_layer_slice(const float* Hs, float* Ws, const float* __restrict__ W, int kbase,
                                                   f32x16 (&acc)[2][COUT / 256]) {
  constexpr int NI = COUT / 256;
  constexpr int LDW = COUT + 4;                  // 16 k x 4 rows of one staging write land in 64 different banks
  constexpr int WPT = COUT * kBK2 / kNT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kh = lane >> 5, rl = lane & 31;
  float wr[WPT];
  // element e = tid + 512 i of a tile is row e / 16 of W, k e % 16 (16 lanes read 64 consecutive bytes): one per-lane offset for
  // all of them, the rest of the address is uniform
  const unsigned voff = (unsigned)(tid >> 4) * LDG + (tid & 15);
  auto fetch = [&](int k0) {
    const float* __restrict__ wk = W + kbase + k0;
#pragma unroll
    for (int i = 0; i < WPT; ++i) wr[i] = (wk + (size_t)i * (kNT / 16) * LDG)[voff];
  };
  fetch(0);
  for (int k0 = 0; k0 < kHK; k0 += kBK2) {
    __syncthreads();                             // the previous tile is consumed (first pass: Hs is complete)
#pragma unroll
    for (int i = 0; i < WPT; ++i) {
      const int e = tid + kNT * i;
      Ws[(e & 15) * LDW + (e >> 4)] = wr[i];
    }
    __syncthreads();
    if (k0 + kBK2 < kHK) fetch(k0 + kBK2);
#pragma unroll
    for (int kk = 0; kk < kBK2; kk += 2) {
      float a[2], b[NI];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = Hs[(k0 + kk + kh) * kLDH + 32 * i + rl];
#pragma unroll
      for (int j = 0; j < NI; ++j) b[j] = Ws[(kk + kh) * LDW + wave * (32 * NI) + 32 * j + rl];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }
  __syncthreads();                               // Hs and Ws may be rewritten
}

// ------------------------------------------------------------------------------------------------------------------
// two-layer MLP + maximum over the points
// ------------------------------------------------------------------------------------------------------------------
struct MlpShape {
  int N, tiles;
  long long shift_stride;                        // floats between the shift1 rows of two clouds (0: one shared row)
};

// The body of both kernels below.  ARG: also report, per column, the lowest row of the tile that attains the tile's maximum
// (-1 when no row compares equal to it, i.e. every valid row is NaN), through tile_arg.
template <int CIN, int H, int COUT, bool ARG>
__device__ __forceinline__ void mlp2_tile(const float* __restrict__ x, const float* __restrict__ W1,
                                          const float* __restrict__ shift1, const float* __restrict__ W2,
                                          const float* __restrict__ b2, float* __restrict__ tile_max,
                                          int* __restrict__ tile_arg, float* __restrict__ y, const MlpShape& s) {
  static_assert(H % kHK == 0 && COUT % 256 == 0 && COUT <= 1024, "eight waves of 32 * NI columns each");
  constexpr int BK1 = CIN >= 32 ? 32 : 4;        // k per staged tile of the first layer
  constexpr int CINP = (CIN + BK1 - 1) / BK1 * BK1;
  constexpr int LDW1 = kHK + 1;
  constexpr int XPT = (kT * BK1 + kNT - 1) / kNT, W1PT = (kHK * BK1 + kNT - 1) / kNT;
  constexpr int NI = COUT / 256;
  __shared__ float Xs[BK1 * kLDH];               // 64 points x BK1 input channels, k-major
  __shared__ float W1s[BK1 * LDW1];              // 128 hidden channels x BK1, k-major
  __shared__ float Hs[kHK * kLDH];               // relu(hidden) of the 64 points, 128 channels, k-major
  __shared__ float Ws[kBK2 * (COUT + 4)];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kh = lane >> 5, rl = lane & 31;
  const int b = blockIdx.x / s.tiles, tile = blockIdx.x - b * s.tiles;
  const int row0 = tile * kT;
  const int rt = wave >> 2, ct = wave & 3;       // first layer: wave = (row tile, 32 hidden channels of the slice)
  const float* __restrict__ xb = x + (size_t)b * s.N * CIN;

  f32x16 acc[2][NI];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int hc0 = 0; hc0 < H; hc0 += kHK) {
    // ---- first layer: hidden[64, hc0 .. hc0 + 128) = x . W1^T ----
    f32x16 acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc1[r] = 0.f;
    float xr[XPT], w1r[W1PT];
    const unsigned w1off = (unsigned)(tid / BK1) * CIN + tid % BK1;
    auto fetch1 = [&](int k0) {
#pragma unroll
      for (int i = 0; i < XPT; ++i) {
        const int e = tid + kNT * i;
        const int r = e / BK1, k = k0 + e % BK1;
        float v = 0.f;
        if (e < kT * BK1 && k < CIN) v = xb[(size_t)min(row0 + r, s.N - 1) * CIN + k];   // rows past N repeat the last one
        xr[i] = v;
      }
#pragma unroll
      for (int i = 0; i < W1PT; ++i) {
        const int e = tid + kNT * i;
        const int k = k0 + tid % BK1;            // kNT is a multiple of BK1: the k of a thread's elements is the same
        float v = 0.f;
        if (e < kHK * BK1 && k < CIN) v = (W1 + (size_t)(hc0 + i * (kNT / BK1)) * CIN + k0)[w1off];
        w1r[i] = v;
      }
    };
    fetch1(0);
    for (int k0 = 0; k0 < CINP; k0 += BK1) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < XPT; ++i) {
        const int e = tid + kNT * i;
        if (e < kT * BK1) Xs[(e % BK1) * kLDH + e / BK1] = xr[i];
      }
#pragma unroll
      for (int i = 0; i < W1PT; ++i) {
        const int e = tid + kNT * i;
        if (e < kHK * BK1) W1s[(e % BK1) * LDW1 + e / BK1] = w1r[i];
      }
      __syncthreads();
      if (k0 + BK1 < CINP) fetch1(k0 + BK1);
#pragma unroll
      for (int kk = 0; kk < BK1; kk += 2) {
        const float a = Xs[(kk + kh) * kLDH + 32 * rt + rl];
        const float w = W1s[(kk + kh) * LDW1 + 32 * ct + rl];
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, w, acc1, 0, 0, 0);
      }
    }
    {
      const int hc = 32 * ct + rl;
      const float sh = shift1[(size_t)b * s.shift_stride + hc0 + hc];
#pragma unroll
      for (int r = 0; r < 16; ++r) Hs[hc * kLDH + 32 * rt + acc_row(r, lane)] = __builtin_fmaxf(acc1[r] + sh, 0.f);
    }
    // ---- second layer: this slice of k ----
    second_layer_slice<COUT, H>(Hs, Ws, W2, hc0, acc);
  }

  // ---- epilogue: bias, optional store, maximum over the tile's valid rows (a wave holds all 64 rows of its columns) ----
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = wave * (32 * NI) + 32 * j + rl;
    const float bias = b2[col];
    float m = -__builtin_inff();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = row0 + 32 * i + acc_row(r, lane);
        const float v = acc[i][j][r] + bias;
        if (row < s.N) {
          m = __builtin_fmaxf(m, v);
          if (y) y[((size_t)b * s.N + row) * COUT + col] = v;
        }
      }
    }
    m = __builtin_fmaxf(m, __shfl_xor(m, 32, kWave));
    if (lane < 32) tile_max[((size_t)b * s.tiles + tile) * COUT + col] = m;
    if constexpr (ARG) {
      // a second, comparing pass over the same accumulators: a lane's rows ascend with (i, r), so walking them downwards
      // leaves the lowest match; the other half of the wave holds the other 32 rows of the column.  Rows past N need no test
      // of their own (32 more live comparison masks would not fit the scalar registers): they were computed from a copy of
      // row N - 1, so one of them can match only where N - 1 matches too, and N - 1 is the lower row: the minimum never
      // lands past N.  The clamp below is purely defensive (it keeps arg inside the cloud whatever the hardware does).
      int a = 0x7fffffff;
#pragma unroll
      for (int i = 1; i >= 0; --i) {
#pragma unroll
        for (int r = 15; r >= 0; --r)
          if (acc[i][j][r] + bias == m) a = 32 * i + acc_row(r, lane);
      }
      a = min(a, __shfl_xor(a, 32, kWave));
      if (lane < 32) tile_arg[((size_t)b * s.tiles + tile) * COUT + col] = a == 0x7fffffff ? -1 : min(row0 + a, s.N - 1);
    }
  }
}

template <int CIN, int H, int COUT>
__global__ __launch_bounds__(kNT) void mlp2_max_kernel(const float* __restrict__ x, const float* __restrict__ W1,
                                                       const float* __restrict__ shift1, const float* __restrict__ W2,
                                                       const float* __restrict__ b2, float* __restrict__ tile_max,
                                                       float* __restrict__ y, const MlpShape s) {
  mlp2_tile<CIN, H, COUT, false>(x, W1, shift1, W2, b2, tile_max, nullptr, y, s);
}

// the same block, reporting the arg-max as well (a kernel of its own: the plain one keeps its registers and its name)
template <int CIN, int H, int COUT>
__global__ __launch_bounds__(kNT) void mlp2_argmax_kernel(const float* __restrict__ x, const float* __restrict__ W1,
                                                          const float* __restrict__ shift1, const float* __restrict__ W2,
                                                          const float* __restrict__ b2, float* __restrict__ tile_max,
                                                          int* __restrict__ tile_arg, float* __restrict__ y, const MlpShape s) {
  mlp2_tile<CIN, H, COUT, true>(x, W1, shift1, W2, b2, tile_max, tile_arg, y, s);
}

// pooled[b, c] = max over the tiles of tile_max[b, t, c], t ascending
__global__ __launch_bounds__(256) void tile_max_fold_kernel(const float* __restrict__ tile_max, int tiles, int C, long long total,
                                                            float* __restrict__ pooled) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const long long b = o / C;
  const int c = (int)(o - b * C);
  const float* p = tile_max + (size_t)b * tiles * C + c;
  float m = p[0];
  for (int t = 1; t < tiles; ++t) m = __builtin_fmaxf(m, p[(size_t)t * C]);
  pooled[o] = m;
}

template <int CIN, int H, int COUT>
bool launch_mlp2(const float* x, const float* W1, const float* shift1, const float* W2, const float* b2, float* pooled, float* y,
                 float* workspace, int B, const MlpShape& s, hipStream_t stream) {
  float* tile_max = s.tiles == 1 ? pooled : workspace;
  mlp2_max_kernel<CIN, H, COUT><<<(unsigned)(B * s.tiles), kNT, 0, stream>>>(x, W1, shift1, W2, b2, tile_max, y, s);
  if (!check_launch("houv_mlp2_max")) return false;
  if (s.tiles > 1) {
    const long long total = (long long)B * COUT;
    tile_max_fold_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(workspace, s.tiles, COUT, total, pooled);
    if (!check_launch("houv_mlp2_max")) return false;
  }
  return true;
}

// pooled as tile_max_fold_kernel makes it (the same fmaxf chain, the same bits), and arg[b, c] = the row the first tile that
// attains the maximum reported: a later tile takes over only when strictly greater, or when no earlier tile had a row at all
__global__ __launch_bounds__(256) void tile_argmax_fold_kernel(const float* __restrict__ tile_max, const int* __restrict__ tile_arg,
                                                               int tiles, int C, long long total, float* __restrict__ pooled,
                                                               int* __restrict__ arg) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const long long b = o / C;
  const int c = (int)(o - b * C);
  const float* p = tile_max + (size_t)b * tiles * C + c;
  const int* q = tile_arg + (size_t)b * tiles * C + c;
  float m = p[0];
  int a = q[0];
  for (int t = 1; t < tiles; ++t) {
    const float v = p[(size_t)t * C];
    const int at = q[(size_t)t * C];
    if (v > m || (a < 0 && at >= 0)) a = at;
    m = __builtin_fmaxf(m, v);
  }
  pooled[o] = m;
  arg[o] = a;
}

template <int CIN, int H, int COUT>
bool launch_mlp2_arg(const float* x, const float* W1, const float* shift1, const float* W2, const float* b2, float* pooled,
                     int* arg, float* y, float* workspace, int B, const MlpShape& s, hipStream_t stream) {
  const size_t cells = (size_t)B * s.tiles * COUT;
  float* tile_max = s.tiles == 1 ? pooled : workspace;
  int* tile_arg = s.tiles == 1 ? arg : reinterpret_cast<int*>(workspace + cells);
  mlp2_argmax_kernel<CIN, H, COUT><<<(unsigned)(B * s.tiles), kNT, 0, stream>>>(x, W1, shift1, W2, b2, tile_max, tile_arg, y, s);
  if (!check_launch("houv_mlp2_max_arg")) return false;
  if (s.tiles > 1) {
    const long long total = (long long)B * COUT;
    tile_argmax_fold_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(tile_max, tile_arg, s.tiles, COUT, total, pooled,
                                                                                 arg);
    if (!check_launch("houv_mlp2_max_arg")) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------------------------
// folding stage
// ------------------------------------------------------------------------------------------------------------------
constexpr int kFoldH = 512;
struct FoldShape {
  int nc, scale, nf, tiles;
};

__global__ __launch_bounds__(kNT, 2) void pcn_fold_kernel(const float* __restrict__ coarse, const float* __restrict__ cvec,
                                                          const float* __restrict__ grid, const float* __restrict__ Wgp,
                                                          const float* __restrict__ W2, const float* __restrict__ b2,
                                                          const float* __restrict__ W3, const float* __restrict__ b3,
                                                          float* __restrict__ fine, const FoldShape s) {
  constexpr int NI = kFoldH / 256;
  __shared__ float In[kT][5];                    // per fine point of the tile: grid x, grid y, centre x y z
  __shared__ float Hs[kHK * kLDH];
  __shared__ float Ws[kBK2 * (kFoldH + 4)];
  __shared__ float red[8][kT][3];                // the eight waves' shares of W3 . h2

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl = lane & 31;
  const int b = blockIdx.x / s.tiles, tile = blockIdx.x - b * s.tiles;
  const int f0 = tile * kT;

  if (tid < kT) {
    const int f = min(f0 + tid, s.nf - 1);       // rows past the cloud repeat its last point; they are never stored
    const int c = f / s.scale, g = f - c * s.scale;
    const float* cp = coarse + ((size_t)b * s.nc + c) * 3;
    In[tid][0] = grid[g]; In[tid][1] = grid[s.scale + g];
    In[tid][2] = cp[0]; In[tid][3] = cp[1]; In[tid][4] = cp[2];
  }
  __syncthreads();
  const float g0 = In[lane][0], g1 = In[lane][1], cx = In[lane][2], cy = In[lane][3], cz = In[lane][4];

  f32x16 acc[2][NI];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int hc0 = 0; hc0 < kFoldH; hc0 += kHK) {
    // h1 of the slice: lane = point, the channel is wave-uniform (its six parameters arrive through the scalar cache)
#pragma unroll 4
    for (int i = 0; i < kHK / 8; ++i) {
      const int c = wave + 8 * i;
      const float* w = Wgp + (size_t)(hc0 + c) * 5;
      const float pre = __builtin_fmaf(w[4], cz, __builtin_fmaf(w[3], cy, __builtin_fmaf(w[2], cx, __builtin_fmaf(w[1], g1, w[0] * g0))));
      Hs[c * kLDH + lane] = __builtin_fmaxf(pre + cvec[(size_t)b * kFoldH + hc0 + c], 0.f);
    }
    second_layer_slice<kFoldH, kFoldH>(Hs, Ws, W2, hc0, acc);
  }

  // ---- h2 = relu(acc + b2); the wave's share of W3 . h2 per row: its columns in-lane, then the 32 lanes by a butterfly ----
  float bias[NI], w3[3][NI];
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int col = wave * (32 * NI) + 32 * j + rl;
    bias[j] = b2[col];
#pragma unroll
    for (int d = 0; d < 3; ++d) w3[d][j] = W3[d * kFoldH + col];
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float p[3] = {0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < NI; ++j) {
        const float h2 = __builtin_fmaxf(acc[i][j][r] + bias[j], 0.f);
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] = __builtin_fmaf(w3[d][j], h2, p[d]);
      }
#pragma unroll
      for (int o = 1; o < 32; o <<= 1) {
#pragma unroll
        for (int d = 0; d < 3; ++d) p[d] += __shfl_xor(p[d], o, kWave);
      }
      if (rl == 0) {
        const int row = 32 * i + acc_row(r, lane);
#pragma unroll
        for (int d = 0; d < 3; ++d) red[wave][row][d] = p[d];
      }
    }
  }
  __syncthreads();
  if (tid < kT * 3) {
    const int row = tid / 3, d = tid - 3 * row;
    if (f0 + row < s.nf) {
      float v = red[0][row][d];
#pragma unroll
      for (int w = 1; w < 8; ++w) v += red[w][row][d];
      fine[((size_t)b * s.nf + f0 + row) * 3 + d] = (v + b3[d]) + In[row][2 + d];
    }
  }
}


// ------------------------------------------------------------------------------------------------------------------
// folding stage, backward.  The forward keeps nothing: a workgroup recomputes h1 and h2 of its 64 fine
// points exactly as pcn_fold_kernel does, turns the h2 accumulators into gh2 = (W3^T gfine) * [h2 > 0] in place, and runs a
// second 64 x 512 x 512 pass of the same k-slice scheme over W2^T for gh1 = (gh2 W2) * [h1 > 0].  h1 and the k-major gh2 go to
// the workspace for the one product that needs both in memory (gW2 = sum gh2^T h1, a split-row GEMM); every row reduction leaves
// the kernel as a per-tile partial that a second kernel adds in tile order.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kPartB2 = 0, kPartW3 = 512, kPartCvec = 2048, kPartWgp = 2560, kPartB3 = 5120;
constexpr int kFoldPart = 5124;                  // floats per tile: gb2[512], gW3[3][512], gcvec[512], gWgp[512][5], gb3[3], pad
struct FoldBwShape {
  int nc, scale, nf, tiles;
  long long GP;                                  // leading dimension of the k-major gh2: B * nf rounded up to the GEMM's chunks
};

__global__ __launch_bounds__(kNT) void pcn_fold_bw_kernel(const float* __restrict__ coarse, const float* __restrict__ cvec,
                                                          const float* __restrict__ grid, const float* __restrict__ Wgp,
                                                          const float* __restrict__ W2, const float* __restrict__ W2T,
                                                          const float* __restrict__ b2, const float* __restrict__ W3,
                                                          const float* __restrict__ gfine, float* __restrict__ h1ws,
                                                          float* __restrict__ gh2T, float* __restrict__ part,
                                                          float* __restrict__ gfp, const FoldBwShape s) {
  constexpr int NI = kFoldH / 256;
  __shared__ float In[kT][5];
  __shared__ float Gf[kT][3];                    // gfine of the tile's points, zeros past the cloud
  __shared__ float Hs[kHK * kLDH];
  __shared__ float Ws[kBK2 * (kFoldH + 4)];
  __shared__ float red[8][kT][3];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rl = lane & 31;
  const int b = blockIdx.x / s.tiles, tile = blockIdx.x - b * s.tiles;
  const int f0 = tile * kT;
  const size_t g0 = (size_t)b * s.nf + f0;       // index of the tile's first fine point among all B * nf
  float* __restrict__ P = part + (size_t)blockIdx.x * kFoldPart;

  if (tid < kT) {
    const int f = min(f0 + tid, s.nf - 1);
    const int c = f / s.scale, g = f - c * s.scale;
    const float* cp = coarse + ((size_t)b * s.nc + c) * 3;
    In[tid][0] = grid[g]; In[tid][1] = grid[s.scale + g];
    In[tid][2] = cp[0]; In[tid][3] = cp[1]; In[tid][4] = cp[2];
    const bool valid = f0 + tid < s.nf;
#pragma unroll
    for (int d = 0; d < 3; ++d) Gf[tid][d] = valid ? gfine[(g0 + tid) * 3 + d] : 0.f;
  }
  __syncthreads();
  const float g0x = In[lane][0], g1x = In[lane][1], cx = In[lane][2], cy = In[lane][3], cz = In[lane][4];

  f32x16 acc[2][NI];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- the forward again: h1 per slice (kept in the workspace as rows), h2's accumulators ----
  for (int hc0 = 0; hc0 < kFoldH; hc0 += kHK) {
#pragma unroll 4
    for (int i = 0; i < kHK / 8; ++i) {
      const int c = wave + 8 * i;
      const float* w = Wgp + (size_t)(hc0 + c) * 5;
      const float pre = __builtin_fmaf(w[4], cz, __builtin_fmaf(w[3], cy, __builtin_fmaf(w[2], cx, __builtin_fmaf(w[1], g1x, w[0] * g0x))));
      Hs[c * kLDH + lane] = __builtin_fmaxf(pre + cvec[(size_t)b * kFoldH + hc0 + c], 0.f);
    }
    __syncthreads();
    for (int e = tid; e < kT * kHK; e += kNT) {
      const int row = e / kHK, c = e - row * kHK;
      if (f0 + row < s.nf) h1ws[(g0 + row) * kFoldH + hc0 + c] = Hs[c * kLDH + row];
    }
    second_layer_slice<kFoldH, kFoldH>(Hs, Ws, W2, hc0, acc);
  }

  // ---- gh2 in place of the accumulators; the tile's shares of gb2 and gW3 ----
  {
    float bias[NI], w3[3][NI], sb2[NI], sw3[3][NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = wave * (32 * NI) + 32 * j + rl;
      bias[j] = b2[col];
      sb2[j] = 0.f;
#pragma unroll
      for (int d = 0; d < 3; ++d) { w3[d][j] = W3[d * kFoldH + col]; sw3[d][j] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * i + acc_row(r, lane);
        const float gx = Gf[row][0], gy = Gf[row][1], gz = Gf[row][2];
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          const float pre = acc[i][j][r] + bias[j];
          const float h2 = __builtin_fmaxf(pre, 0.f);
          const float t = __builtin_fmaf(w3[2][j], gz, __builtin_fmaf(w3[1][j], gy, w3[0][j] * gx));
          const float gh2 = pre > 0.f ? t : 0.f;
          acc[i][j][r] = gh2;
          sb2[j] += gh2;
          sw3[0][j] = __builtin_fmaf(gx, h2, sw3[0][j]);
          sw3[1][j] = __builtin_fmaf(gy, h2, sw3[1][j]);
          sw3[2][j] = __builtin_fmaf(gz, h2, sw3[2][j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int col = wave * (32 * NI) + 32 * j + rl;
      sb2[j] += __shfl_xor(sb2[j], 32, kWave);
#pragma unroll
      for (int d = 0; d < 3; ++d) sw3[d][j] += __shfl_xor(sw3[d][j], 32, kWave);
      if (lane < 32) {
        P[kPartB2 + col] = sb2[j];
#pragma unroll
        for (int d = 0; d < 3; ++d) P[kPartW3 + d * kFoldH + col] = sw3[d][j];
      }
    }
  }

  // ---- gh1's accumulators = gh2 . W2: the 128 columns of a slice belong to two waves, which lay them out k-major in Hs ----
  f32x16 acc2[2][NI];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc2[i][j][r] = 0.f;
  for (int hc0 = 0; hc0 < kFoldH; hc0 += kHK) {
    if ((wave >> 1) == hc0 / kHK) {
#pragma unroll
      for (int j = 0; j < NI; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            Hs[((wave & 1) * (32 * NI) + 32 * j + rl) * kLDH + 32 * i + acc_row(r, lane)] = acc[i][j][r];
    }
    __syncthreads();
    for (int e = tid; e < kT * kHK; e += kNT) {
      const int c = e / kT, row = e - c * kT;
      if (f0 + row < s.nf) gh2T[(size_t)(hc0 + c) * s.GP + g0 + row] = Hs[c * kLDH + row];
    }
    second_layer_slice<kFoldH, kFoldH>(Hs, Ws, W2T, hc0, acc2);
  }

  // ---- gh1 = acc2 * [h1 > 0] (h1's sign from the forward's own expression); its shares of gcvec, gWgp and of the centres ----
  {
    float wg[5][NI], cv[NI], scv[NI], swg[5][NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int k = wave * (32 * NI) + 32 * j + rl;
      cv[j] = cvec[(size_t)b * kFoldH + k];
      scv[j] = 0.f;
#pragma unroll
      for (int m = 0; m < 5; ++m) { wg[m][j] = Wgp[(size_t)k * 5 + m]; swg[m][j] = 0.f; }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * i + acc_row(r, lane);
        float u[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) u[m] = In[row][m];
        float p[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NI; ++j) {
          const float pre = __builtin_fmaf(wg[4][j], u[4], __builtin_fmaf(wg[3][j], u[3], __builtin_fmaf(wg[2][j], u[2], __builtin_fmaf(wg[1][j], u[1], wg[0][j] * u[0]))));
          const float gh1 = (pre + cv[j]) > 0.f ? acc2[i][j][r] : 0.f;
          scv[j] += gh1;
#pragma unroll
          for (int m = 0; m < 5; ++m) swg[m][j] = __builtin_fmaf(gh1, u[m], swg[m][j]);
#pragma unroll
          for (int d = 0; d < 3; ++d) p[d] = __builtin_fmaf(wg[2 + d][j], gh1, p[d]);
        }
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
#pragma unroll
          for (int d = 0; d < 3; ++d) p[d] += __shfl_xor(p[d], o, kWave);
        }
        if (rl == 0) {
#pragma unroll
          for (int d = 0; d < 3; ++d) red[wave][row][d] = p[d];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int k = wave * (32 * NI) + 32 * j + rl;
      scv[j] += __shfl_xor(scv[j], 32, kWave);
#pragma unroll
      for (int m = 0; m < 5; ++m) swg[m][j] += __shfl_xor(swg[m][j], 32, kWave);
      if (lane < 32) {
        P[kPartCvec + k] = scv[j];
#pragma unroll
        for (int m = 0; m < 5; ++m) P[kPartWgp + k * 5 + m] = swg[m][j];
      }
    }
  }
  __syncthreads();
  if (tid < kT * 3) {
    const int row = tid / 3, d = tid - 3 * row;
    if (f0 + row < s.nf) {
      float v = red[0][row][d];
#pragma unroll
      for (int w = 1; w < 8; ++w) v += red[w][row][d];
      gfp[(g0 + row) * 3 + d] = Gf[row][d] + v;  // the centre path plus the Wgp[:, 2:5] path of this fine point
    }
  }
  if (tid < 3) {
    float v = 0.f;
    for (int row = 0; row < kT; ++row) v += Gf[row][tid];
    P[kPartB3 + tid] = v;
  }
}

// out[g * n + o] = sum over t < T of part[(g * T + t) * kFoldPart + off + o], t ascending (blockIdx.y = g)
__global__ __launch_bounds__(256) void fold_bw_sum_kernel(const float* __restrict__ part, int T, int off, int n, float* __restrict__ out) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n) return;
  const float* p = part + (size_t)blockIdx.y * T * kFoldPart + off + o;
  float v = p[0];
#pragma unroll 8                                 // eight tiles' loads in flight; the additions keep their order
  for (int t = 1; t < T; ++t) v += p[(size_t)t * kFoldPart];
  out[(size_t)blockIdx.y * n + o] = v;
}

// out[i] = sum over k < S of part[k * n + i], k ascending
__global__ __launch_bounds__(256) void fold_bw_chunks_kernel(const float* __restrict__ part, int S, int n, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v = part[i];
  for (int k = 1; k < S; ++k) v += part[(size_t)k * n + i];
  out[i] = v;
}

// gcoarse[b, c, d] = sum over the scale cells j of gfp[b, c * scale + j, d], j ascending (o runs over B * nc * 3)
__global__ __launch_bounds__(256) void fold_bw_coarse_kernel(const float* __restrict__ gfp, int scale, long long total,
                                                             float* __restrict__ gcoarse) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= total) return;
  const long long c = o / 3;
  const int d = (int)(o - c * 3);
  const float* p = gfp + (size_t)c * scale * 3 + d;
  float v = p[0];
  for (int j = 1; j < scale; ++j) v += p[(size_t)j * 3];
  gcoarse[o] = v;
}

__global__ __launch_bounds__(256) void fold_bw_transpose_kernel(const float* __restrict__ W, float* __restrict__ WT) {
  const int o = blockIdx.x * 256 + threadIdx.x;  // kFoldH * kFoldH elements
  const int n = o / kFoldH, c = o - n * kFoldH;
  WT[o] = W[(size_t)c * kFoldH + n];
}

struct FoldBwLayout {                            // offsets into the workspace in floats, each a multiple of 4
  long long W2T, h1, gh2T, part, gfp, gW2p, total;
  long long G, GP;
  int KC, SK, tiles;
};

FoldBwLayout fold_bw_layout(int B, int nc, int scale) {
  FoldBwLayout l;
  const long long nf = (long long)nc * scale;
  l.tiles = (int)((nf + kT - 1) / kT);
  l.G = (long long)B * nf;
  // gW2 = gh2^T h1 has a 512 x 512 output and a reduction over all B * nf fine points: about 32 chunks of rows over the GEMM's
  // outer dimension (16 output tiles each) fill the device; chunks are multiples of 32 rows so that full tiles stay aligned
  l.KC = (int)std::max<long long>(32, ((l.G + 31) / 32 + 31) / 32 * 32);
  l.SK = (int)((l.G + l.KC - 1) / l.KC);
  l.GP = (long long)l.SK * l.KC;
  auto up4 = [](long long n) { return (n + 3) & ~3LL; };
  long long o = 0;
  l.W2T = o; o += (long long)kFoldH * kFoldH;
  l.h1 = o; o += l.GP * kFoldH;
  l.gh2T = o; o += l.GP * kFoldH;
  l.part = o; o += up4((long long)B * l.tiles * kFoldPart);
  l.gfp = o; o += up4(l.G * 3);
  l.gW2p = o; o += (long long)l.SK * kFoldH * kFoldH;
  l.total = o;
  return l;
}

const char* fold_bw_check(int B, int nc, int scale) {
  static thread_local char msg[200];
  if (B < 0 || nc < 1 || scale < 1) {
    snprintf(msg, sizeof msg, "bad shape B=%d nc=%d scale=%d (nc, scale >= 1)", B, nc, scale);
    return msg;
  }
  const long long nf = (long long)nc * scale, tiles = (nf + kT - 1) / kT;
  if (nf > 0x7fffffffLL || (long long)B * tiles > 0x7fffffffLL || (long long)B * nf > (1LL << 30)) {
    snprintf(msg, sizeof msg, "B=%d x nc=%d x scale=%d is too many fine points for one launch", B, nc, scale);
    return msg;
  }
  return nullptr;
}

}  // namespace
}  // namespace houv

extern "C" long long houv_mlp2_max_workspace_bytes(int B, int N, int Cout) {
  if (B <= 0 || N <= 0 || Cout <= 0) return 0;
  const long long tiles = ((long long)N + houv::kT - 1) / houv::kT;
  return tiles > 1 ? (long long)B * tiles * Cout * (long long)sizeof(float) : 0;
}

namespace houv {
namespace {
// the checks and the dispatch of houv_mlp2_max and houv_mlp2_max_arg (`fn` names the caller in messages; arg: the latter only)
int mlp2_entry(const char* fn, bool want_arg, const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
               long long shift1_stride, const float* W2, const float* b2, int Cout, float* pooled, int* arg, float* y_or_null,
               float* workspace, void* stream) {
  if (B < 0 || N < 1) {
    set_error("%s: bad shape B=%d N=%d (N >= 1)", fn, B, N);
    return 0;
  }
  const bool first = Cin == 3 && H == 128 && Cout == 256, second = Cin == 256 && H == 512 && Cout == 1024;
  if (!first && !second) {
    set_error("%s: (Cin, H, Cout) = (%d, %d, %d) has no kernel: (3, 128, 256) and (256, 512, 1024) are served", fn, Cin, H, Cout);
    return 0;
  }
  if (shift1_stride != 0 && shift1_stride < H) {
    set_error("%s: shift1_stride=%lld must be 0 (one shared row) or >= H=%d", fn, shift1_stride, H);
    return 0;
  }
  const long long tiles = ((long long)N + kT - 1) / kT;
  if ((long long)B * tiles > 0x7fffffffLL) {
    set_error("%s: B=%d x N=%d is too many row tiles", fn, B, N);
    return 0;
  }
  if (B == 0) return 1;
  {
    const void* req[] = {x, W1, shift1, W2, b2, pooled, arg};
    const char* names[] = {"x", "W1", "shift1", "W2", "b2", "pooled", "arg"};
    for (int i = 0; i < (want_arg ? 7 : 6); ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  if (tiles > 1 && !workspace) {
    set_error("%s: workspace is a null pointer: N=%d spans %lld row tiles (%s_workspace_bytes)", fn, N, tiles, fn);
    return 0;
  }
  const MlpShape s{N, (int)tiles, shift1_stride};
  hipStream_t st = (hipStream_t)stream;
  bool ok;
  if (want_arg)
    ok = first ? launch_mlp2_arg<3, 128, 256>(x, W1, shift1, W2, b2, pooled, arg, y_or_null, workspace, B, s, st)
               : launch_mlp2_arg<256, 512, 1024>(x, W1, shift1, W2, b2, pooled, arg, y_or_null, workspace, B, s, st);
  else
    ok = first ? launch_mlp2<3, 128, 256>(x, W1, shift1, W2, b2, pooled, y_or_null, workspace, B, s, st)
               : launch_mlp2<256, 512, 1024>(x, W1, shift1, W2, b2, pooled, y_or_null, workspace, B, s, st);
  return ok ? 1 : 0;
}
}  // namespace
}  // namespace houv

extern "C" int houv_mlp2_max(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
                             long long shift1_stride, const float* W2, const float* b2, int Cout, float* pooled,
                             float* y_or_null, float* workspace, void* stream) {
  return houv::mlp2_entry("houv_mlp2_max", false, x, B, N, Cin, W1, H, shift1, shift1_stride, W2, b2, Cout, pooled, nullptr,
                          y_or_null, workspace, stream);
}

extern "C" long long houv_mlp2_max_arg_workspace_bytes(int B, int N, int Cout) {
  return 2 * houv_mlp2_max_workspace_bytes(B, N, Cout);     // the per-tile maxima, then the per-tile rows
}

extern "C" int houv_mlp2_max_arg(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
                                 long long shift1_stride, const float* W2, const float* b2, int Cout, float* pooled, int32_t* arg,
                                 float* y_or_null, float* workspace, void* stream) {
  return houv::mlp2_entry("houv_mlp2_max_arg", true, x, B, N, Cin, W1, H, shift1, shift1_stride, W2, b2, Cout, pooled, arg,
                          y_or_null, workspace, stream);
}

extern "C" int houv_pcn_fold(const float* coarse, const float* cvec, const float* grid, int B, int nc, int scale,
                             const float* Wgp, const float* W2, const float* b2, const float* W3, const float* b3, float* fine,
                             void* stream) {
  using namespace houv;
  if (B < 0 || nc < 1 || scale < 1) {
    set_error("houv_pcn_fold: bad shape B=%d nc=%d scale=%d (nc, scale >= 1)", B, nc, scale);
    return 0;
  }
  const long long nf = (long long)nc * scale;
  const long long tiles = (nf + kT - 1) / kT;
  if (nf > 0x7fffffffLL || (long long)B * tiles > 0x7fffffffLL) {
    set_error("houv_pcn_fold: B=%d x nc=%d x scale=%d is too many fine points for one launch", B, nc, scale);
    return 0;
  }
  if (B == 0) return 1;
  {
    const void* req[] = {coarse, cvec, grid, Wgp, W2, b2, W3, b3, fine};
    const char* names[] = {"coarse", "cvec", "grid", "Wgp", "W2", "b2", "W3", "b3", "fine"};
    for (int i = 0; i < 9; ++i)
      if (!req[i]) {
        set_error("houv_pcn_fold: %s is a null pointer", names[i]);
        return 0;
      }
  }
  const FoldShape s{nc, scale, (int)nf, (int)tiles};
  pcn_fold_kernel<<<(unsigned)(B * tiles), kNT, 0, (hipStream_t)stream>>>(coarse, cvec, grid, Wgp, W2, b2, W3, b3, fine, s);
  return check_launch("houv_pcn_fold") ? 1 : 0;
}

extern "C" long long houv_pcn_fold_backward_workspace_bytes(int B, int nc, int scale) {
  using namespace houv;
  if (B <= 0 || fold_bw_check(B, nc, scale)) return 0;
  return fold_bw_layout(B, nc, scale).total * 4;
}

extern "C" int houv_pcn_fold_backward(const float* coarse, const float* cvec, const float* grid, int B, int nc, int scale,
                                      const float* Wgp, const float* W2, const float* b2, const float* W3, const float* b3,
                                      const float* gfine, float* gcoarse, float* gcvec, float* gWgp, float* gW2, float* gb2,
                                      float* gW3, float* gb3, void* workspace, long long workspace_bytes, void* stream) {
  using namespace houv;
  const char* fn = "houv_pcn_fold_backward";
  if (const char* why = fold_bw_check(B, nc, scale)) {
    set_error("%s: %s", fn, why);
    return 0;
  }
  {
    const void* req[] = {coarse, cvec, grid, Wgp, W2, b2, W3, b3, gfine, gcoarse, gcvec, gWgp, gW2, gb2, gW3, gb3};
    const char* names[] = {"coarse", "cvec", "grid", "Wgp", "W2", "b2", "W3", "b3", "gfine", "gcoarse", "gcvec", "gWgp", "gW2", "gb2", "gW3", "gb3"};
    for (int i = 0; i < 16; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {                                  // no cloud: the weight gradients are zero
    bool ok = hipMemsetAsync(gWgp, 0, kFoldH * 5 * 4, st) == hipSuccess && hipMemsetAsync(gW2, 0, (size_t)kFoldH * kFoldH * 4, st) == hipSuccess &&
              hipMemsetAsync(gb2, 0, kFoldH * 4, st) == hipSuccess && hipMemsetAsync(gW3, 0, 3 * kFoldH * 4, st) == hipSuccess &&
              hipMemsetAsync(gb3, 0, 3 * 4, st) == hipSuccess;
    if (!ok) set_error("%s: hipMemsetAsync failed", fn);
    return ok ? 1 : 0;
  }
  const FoldBwLayout l = fold_bw_layout(B, nc, scale);
  if (!workspace || workspace_bytes < l.total * 4) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed (houv_pcn_fold_backward_workspace_bytes)", fn, workspace_bytes,
              workspace, l.total * 4);
    return 0;
  }
  float* w = static_cast<float*>(workspace);
  float *W2T = w + l.W2T, *h1 = w + l.h1, *gh2T = w + l.gh2T, *part = w + l.part, *gfp = w + l.gfp, *gW2p = w + l.gW2p;
  const long long pad = l.GP - l.G;
  if (pad > 0) {                                 // the rows past B * nf of the last chunk take part in the GEMM: zeros
    if (hipMemsetAsync(h1 + l.G * kFoldH, 0, (size_t)pad * kFoldH * 4, st) != hipSuccess ||
        hipMemset2DAsync(gh2T + l.G, (size_t)l.GP * 4, 0, (size_t)pad * 4, kFoldH, st) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", fn);
      return 0;
    }
  }
  fold_bw_transpose_kernel<<<kFoldH * kFoldH / 256, 256, 0, st>>>(W2, W2T);
  if (!check_launch(fn)) return 0;
  const FoldBwShape s{nc, scale, nc * scale, l.tiles, l.GP};
  const int T = B * l.tiles;
  pcn_fold_bw_kernel<<<(unsigned)T, kNT, 0, st>>>(coarse, cvec, grid, Wgp, W2, W2T, b2, W3, gfine, h1, gh2T, part, gfp, s);
  if (!check_launch(fn)) return 0;
  const struct { int groups, T, off, n; float* out; } sums[] = {{1, T, kPartB2, kFoldH, gb2},
                                                                {1, T, kPartW3, 3 * kFoldH, gW3},
                                                                {1, T, kPartWgp, 5 * kFoldH, gWgp},
                                                                {1, T, kPartB3, 3, gb3},
                                                                {B, l.tiles, kPartCvec, kFoldH, gcvec}};
  for (const auto& q : sums) {
    fold_bw_sum_kernel<<<dim3((unsigned)((q.n + 255) / 256), (unsigned)q.groups), 256, 0, st>>>(part, q.T, q.off, q.n, q.out);
    if (!check_launch(fn)) return 0;
  }
  const long long nco = (long long)B * nc * 3;
  fold_bw_coarse_kernel<<<(unsigned)((nco + 255) / 256), 256, 0, st>>>(gfp, scale, nco, gcoarse);
  if (!check_launch(fn)) return 0;
  // gW2 = gh2^T h1: the fine points split into SK chunks over the GEMM's outer dimension, the partials added chunks ascending
  if (!houv_gemm_f32(gh2T, h1, gW2p, kFoldH, kFoldH, l.KC, (int)l.GP, kFoldH, kFoldH, 0, l.SK, 1, l.KC, 0, (long long)l.KC * kFoldH, 0,
                     (long long)kFoldH * kFoldH, 0, 1.f, nullptr, nullptr, nullptr, 0, 0, 0, 0, stream))
    return 0;
  fold_bw_chunks_kernel<<<kFoldH * kFoldH / 256, 256, 0, st>>>(gW2p, l.SK, kFoldH * kFoldH, gW2);
  return check_launch(fn) ? 1 : 0;
}
