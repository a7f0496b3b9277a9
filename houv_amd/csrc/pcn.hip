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

template <int CIN, int H, int COUT>
__global__ __launch_bounds__(kNT) void mlp2_max_kernel(const float* __restrict__ x, const float* __restrict__ W1,
                                                       const float* __restrict__ shift1, const float* __restrict__ W2,
                                                       const float* __restrict__ b2, float* __restrict__ tile_max,
                                                       float* __restrict__ y, const MlpShape s) {
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
  }
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

}  // namespace
}  // namespace houv

extern "C" long long houv_mlp2_max_workspace_bytes(int B, int N, int Cout) {
  if (B <= 0 || N <= 0 || Cout <= 0) return 0;
  const long long tiles = ((long long)N + houv::kT - 1) / houv::kT;
  return tiles > 1 ? (long long)B * tiles * Cout * (long long)sizeof(float) : 0;
}

extern "C" int houv_mlp2_max(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
                             long long shift1_stride, const float* W2, const float* b2, int Cout, float* pooled,
                             float* y_or_null, float* workspace, void* stream) {
  using namespace houv;
  if (B < 0 || N < 1) {
    set_error("houv_mlp2_max: bad shape B=%d N=%d (N >= 1)", B, N);
    return 0;
  }
  const bool first = Cin == 3 && H == 128 && Cout == 256, second = Cin == 256 && H == 512 && Cout == 1024;
  if (!first && !second) {
    set_error("houv_mlp2_max: (Cin, H, Cout) = (%d, %d, %d) has no kernel: (3, 128, 256) and (256, 512, 1024) are served", Cin, H,
              Cout);
    return 0;
  }
  if (shift1_stride != 0 && shift1_stride < H) {
    set_error("houv_mlp2_max: shift1_stride=%lld must be 0 (one shared row) or >= H=%d", shift1_stride, H);
    return 0;
  }
  const long long tiles = ((long long)N + kT - 1) / kT;
  if ((long long)B * tiles > 0x7fffffffLL) {
    set_error("houv_mlp2_max: B=%d x N=%d is too many row tiles", B, N);
    return 0;
  }
  if (B == 0) return 1;
  {
    const void* req[] = {x, W1, shift1, W2, b2, pooled};
    const char* names[] = {"x", "W1", "shift1", "W2", "b2", "pooled"};
    for (int i = 0; i < 6; ++i)
      if (!req[i]) {
        set_error("houv_mlp2_max: %s is a null pointer", names[i]);
        return 0;
      }
  }
  if (tiles > 1 && !workspace) {
    set_error("houv_mlp2_max: workspace is a null pointer: N=%d spans %lld row tiles (houv_mlp2_max_workspace_bytes)", N, tiles);
    return 0;
  }
  const MlpShape s{N, (int)tiles, shift1_stride};
  const bool ok = first ? launch_mlp2<3, 128, 256>(x, W1, shift1, W2, b2, pooled, y_or_null, workspace, B, s, (hipStream_t)stream)
                        : launch_mlp2<256, 512, 1024>(x, W1, shift1, W2, b2, pooled, y_or_null, workspace, B, s, (hipStream_t)stream);
  return ok ? 1 : 0;
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
