// idam.hip -- the two device pieces of the IDAM head (registration/models/idam.py) that a composition of tensor ops does worst:
//
//   houv_idam_simmat   one iteration's whole similarity stage (:267-320): the [B, 2E+4, M, M] pair tensor, the four 1x1 Conv2d
//                      layers over it, the row maximum after the second and the row arg-max after the fourth, fused.  A pair
//                      (i, j) lives in ONE lane from its distance to its score: no [., M, M] tensor reaches memory unless the
//                      caller asks for the scores.  The first layer splits into a per-row term W1[:, :E] es_i, a per-column term
//                      W1[:, E:2E] et_j and a 4-wide pair term; the two projections are computed in the workgroup (rows once,
//                      columns once per staged chunk) and kept in registers / LDS.  The two 32x32 layers are plain fp32 FMAs
//                      whose weights are wave-uniform and arrive through the scalar cache.
//   houv_edge_diff     Propagate's edge features (:121-124): X[idx] - X, written with a leading dimension so that a 3-channel
//                      input feeds the GEMM with an aligned stride.
//
// Arithmetic is fp32 with fixed expression trees (-ffp-contract=off, explicit fma); nothing here allocates or uses atomics, and
// every reduction runs in a fixed order, so results are bit-identical from call to call.
#include "houv_common.h"

namespace houv {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// similarity matrix
// ------------------------------------------------------------------------------------------------------------------
constexpr int kSimBlock = 256;                   // 4 waves
constexpr int kSimRows = 16;                     // source rows per workgroup: row = lane >> 2
constexpr int kSimSlots = 16;                    // column slots per workgroup: slot = 4 * wave + (lane & 3)
constexpr int kSimChunk = 128;                   // target columns staged in LDS per pass: 8 per slot
constexpr int kSimH = 32;                        // hidden width of the four layers
constexpr int kSimQLd = kSimH + 4;               // LDS row stride of the column projections: the 4 rows a wave reads at once sit in
                                                 // different banks
constexpr int kSimMaxE = 128;

// every pointer is its own __restrict__ kernel argument: the read-only, wave-uniform weight loads then go through the scalar cache
struct SimShape {
  int Ms, Mt, E, tiles;
};

__global__ __launch_bounds__(kSimBlock, 2) void idam_simmat_kernel(
    const float* __restrict__ g_src, const float* __restrict__ g_tgt, const float* __restrict__ g_es, const float* __restrict__ g_et,
    const float* __restrict__ g_W1, const float* __restrict__ g_s1, const float* __restrict__ g_t1, const float* __restrict__ g_W2,
    const float* __restrict__ g_b2, const float* __restrict__ g_W3, const float* __restrict__ g_s3, const float* __restrict__ g_t3,
    const float* __restrict__ g_w4, const float* __restrict__ g_b4, float* __restrict__ g_rowmax, int32_t* __restrict__ g_corr_idx,
    float* __restrict__ g_corr, float* __restrict__ g_scores, const SimShape a) {
  __shared__ __attribute__((aligned(16))) float Qs[kSimChunk][kSimQLd];   // W1[:, E:2E] . et_j of the staged columns
  __shared__ __attribute__((aligned(16))) float Ts[kSimChunk][4];         // their coordinates
  __shared__ float Ps[kSimRows][kSimH + 1];                               // W1[:, :E] . es_i of the workgroup's rows
  __shared__ __attribute__((aligned(16))) float Wp[kSimH][12];             // per channel: W1[c, 2E..2E+3] (d, ux, uy, uz), s1, t1, b2, s3, t3, w4
  __shared__ float redm[4][kSimRows][kSimH + 1];                          // per-wave row maxima, then the four waves' combine
  __shared__ float reds[4][kSimRows];
  __shared__ int redj[4][kSimRows];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / a.tiles, tile = blockIdx.x % a.tiles;
  const int Ms = a.Ms, Mt = a.Mt, E = a.E;
  const int ld1 = 2 * E + 4;
  const int row = lane >> 2;
  const int slot = (wave << 2) | (lane & 3);
  const int i = tile * kSimRows + row;
  const bool row_ok = i < Ms;
  const int ic = row_ok ? i : Ms - 1;

  // ---- row projections: 16 rows x 32 channels, two channels per thread ----
  {
    const int r = tid & (kSimRows - 1);
    const int c0 = (tid >> 4) * 2;
    const int ir = min(tile * kSimRows + r, Ms - 1);
    const float4* e4 = reinterpret_cast<const float4*>(g_es + ((size_t)b * Ms + ir) * E);
    const float* w0 = g_W1 + (size_t)c0 * ld1;
    const float* w1 = w0 + ld1;
    float p0 = 0.f, p1 = 0.f;
    for (int e = 0; e < E; e += 4) {
      const float4 v = e4[e >> 2];
      p0 = __builtin_fmaf(w0[e + 3], v.w, __builtin_fmaf(w0[e + 2], v.z, __builtin_fmaf(w0[e + 1], v.y, __builtin_fmaf(w0[e], v.x, p0))));
      p1 = __builtin_fmaf(w1[e + 3], v.w, __builtin_fmaf(w1[e + 2], v.z, __builtin_fmaf(w1[e + 1], v.y, __builtin_fmaf(w1[e], v.x, p1))));
    }
    Ps[r][c0] = p0;
    Ps[r][c0 + 1] = p1;
    if (tid < kSimH) {      // the row stride of W1 is a run-time value: staged once, these are read at fixed LDS offsets
      const float* wp = g_W1 + (size_t)tid * ld1 + 2 * E;
      *reinterpret_cast<float4*>(&Wp[tid][0]) = make_float4(wp[0], wp[1], wp[2], wp[3]);
      *reinterpret_cast<float4*>(&Wp[tid][4]) = make_float4(g_s1[tid], g_t1[tid], g_b2[tid], g_s3[tid]);
      *reinterpret_cast<float4*>(&Wp[tid][8]) = make_float4(g_t3[tid], g_w4[tid], 0.f, 0.f);
    }
  }
  __syncthreads();
  float P[kSimH], rm[kSimH];
#pragma unroll
  for (int c = 0; c < kSimH; ++c) { P[c] = Ps[row][c]; rm[c] = -__builtin_inff(); }
  const float* sp = g_src + ((size_t)b * Ms + ic) * 3;
  const float sx = sp[0], sy = sp[1], sz = sp[2];
  float best = -__builtin_inff();
  int bj = 0x7fffffff;
  const float b4 = g_b4[0];

  for (int chunk0 = 0; chunk0 < Mt; chunk0 += kSimChunk) {
    __syncthreads();                                 // the previous chunk has been consumed
    // ---- column projections of the chunk: thread = (column, half of the channels); the half is wave-uniform ----
    {
      const int jl = tid & (kSimChunk - 1);
      const int ch0 = (tid >> 7) * 16;
      const int j = min(chunk0 + jl, Mt - 1);
      const float4* e4 = reinterpret_cast<const float4*>(g_et + ((size_t)b * Mt + j) * E);
      const float* w = g_W1 + (size_t)ch0 * ld1 + E;
      float q[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) q[c] = 0.f;
      for (int e = 0; e < E; e += 4) {
        const float4 v = e4[e >> 2];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
          const float* wc = w + (size_t)c * ld1 + e;
          q[c] = __builtin_fmaf(wc[3], v.w, __builtin_fmaf(wc[2], v.z, __builtin_fmaf(wc[1], v.y, __builtin_fmaf(wc[0], v.x, q[c]))));
        }
      }
#pragma unroll
      for (int c = 0; c < 16; c += 4) *reinterpret_cast<float4*>(&Qs[jl][ch0 + c]) = make_float4(q[c], q[c + 1], q[c + 2], q[c + 3]);
      if (tid < kSimChunk) {
        const float* tp = g_tgt + ((size_t)b * Mt + j) * 3;
        *reinterpret_cast<float4*>(&Ts[jl][0]) = make_float4(tp[0], tp[1], tp[2], 0.f);
      }
    }
    __syncthreads();

#pragma unroll 1
    for (int t = 0; t < kSimChunk / kSimSlots; ++t) {
      const int jl = slot + kSimSlots * t;
      const int j = chunk0 + jl;
      if (j >= Mt) break;                            // j grows with t: nothing further in this chunk for this lane
      // the per-channel table is re-read every pass through an offset the optimiser cannot see through: hoisted out of the loop
      // its 320 values join the 128 live ones (P, rm, h1, h2) and no longer fit the 256 VGPRs of the two waves per SIMD this
      // kernel is built for (__launch_bounds__(256, 2)); tests/test_idam_kernel_resources.py holds the register count
      int lz = 0;
      asm volatile("" : "+v"(lz));
      const float(*Wc)[12] = reinterpret_cast<const float(*)[12]>(&Wp[0][0] + lz);
      const float4 tj = *reinterpret_cast<const float4*>(&Ts[jl][0]);
      const float dx = sx - tj.x, dy = sy - tj.y, dz = sz - tj.z;
      const float d = sqrtf((dx * dx + dy * dy) + dz * dz);
      const float den = d + 1e-8f;
      const float ux = dx / den, uy = dy / den, uz = dz / den;
      float h1[kSimH], h2[kSimH];
#pragma unroll
      for (int c4 = 0; c4 < kSimH; c4 += 4) {
        const float4 qv = *reinterpret_cast<const float4*>(&Qs[jl][c4]);
        const float qa[4] = {qv.x, qv.y, qv.z, qv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = c4 + u;
          const float4 wp = *reinterpret_cast<const float4*>(&Wc[c][0]);
          const float2 st = *reinterpret_cast<const float2*>(&Wc[c][4]);
          const float pair = __builtin_fmaf(wp.w, uz, __builtin_fmaf(wp.z, uy, __builtin_fmaf(wp.y, ux, wp.x * d)));
          const float pre = (P[c] + qa[u]) + pair;
          h1[c] = __builtin_fmaxf(__builtin_fmaf(st.x, pre, st.y), 0.f);
        }
      }
#pragma unroll
      for (int c = 0; c < kSimH; ++c) {
        float acc = Wc[c][6];
#pragma unroll
        for (int k = 0; k < kSimH; ++k) acc = __builtin_fmaf(g_W2[c * kSimH + k], h1[k], acc);
        h2[c] = acc;
        rm[c] = __builtin_fmaxf(rm[c], acc);
      }
      float sc = b4;
#pragma unroll
      for (int c = 0; c < kSimH; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < kSimH; ++k) acc = __builtin_fmaf(g_W3[c * kSimH + k], h2[k], acc);
        const float h3 = __builtin_fmaxf(__builtin_fmaf(Wc[c][7], acc, Wc[c][8]), 0.f);
        sc = __builtin_fmaf(Wc[c][9], h3, sc);
      }
      sc = sc < -20.f ? -20.f : (sc > 20.f ? 20.f : sc);
      if (g_scores && row_ok) g_scores[((size_t)b * Ms + i) * Mt + j] = sc;
      if (sc > best) { best = sc; bj = j; }          // j ascends within a lane: the first of equal scores stays
    }
  }

  // ---- combine the 16 column slots of every row: 4 lanes by shuffles, then the 4 waves through LDS; fixed order ----
#pragma unroll
  for (int o = 1; o <= 2; o <<= 1) {
#pragma unroll
    for (int c = 0; c < kSimH; ++c) rm[c] = __builtin_fmaxf(rm[c], __shfl_xor(rm[c], o, kWave));
    const float ob = __shfl_xor(best, o, kWave);
    const int oj = __shfl_xor(bj, o, kWave);
    if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
  }
  if ((lane & 3) == 0) {
#pragma unroll
    for (int c = 0; c < kSimH; ++c) redm[wave][row][c] = rm[c];
    reds[wave][row] = best;
    redj[wave][row] = bj;
  }
  __syncthreads();
  if (g_rowmax) {
    for (int o = tid; o < kSimRows * kSimH; o += kSimBlock) {
      const int r = o / kSimH, c = o % kSimH;
      const int io = tile * kSimRows + r;
      if (io < Ms) {
        const float m = __builtin_fmaxf(__builtin_fmaxf(redm[0][r][c], redm[1][r][c]), __builtin_fmaxf(redm[2][r][c], redm[3][r][c]));
        g_rowmax[((size_t)b * Ms + io) * kSimH + c] = m;
      }
    }
  }
  if (tid < kSimRows && tile * kSimRows + tid < Ms) {
    const int io = tile * kSimRows + tid;
    float bs = reds[0][tid];
    int j = redj[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      const float ob = reds[w][tid];
      const int oj = redj[w][tid];
      if (ob > bs || (ob == bs && oj < j)) { bs = ob; j = oj; }
    }
    if (j < 0 || j >= Mt) j = 0;                     // a row whose scores are all NaN
    if (g_corr_idx) g_corr_idx[(size_t)b * Ms + io] = j;
    if (g_corr) {
      const float* tp = g_tgt + ((size_t)b * Mt + j) * 3;
      float* o = g_corr + (size_t)b * 3 * Ms + io;
      o[0] = tp[0]; o[Ms] = tp[1]; o[2 * (size_t)Ms] = tp[2];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// edge differences
// ------------------------------------------------------------------------------------------------------------------
constexpr int kEdgeBlock = 256;

// one thread per V output columns of one (point, neighbour) row; V = 4 moves 16 bytes at a time
template <int V>
__global__ __launch_bounds__(kEdgeBlock) void edge_diff_kernel(const float* __restrict__ X, const int32_t* __restrict__ idx,
                                                               long long total, int N, int k, int C, int idx_ld, int ldo,
                                                               float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * kEdgeBlock + threadIdx.x;
  if (e >= total) return;
  const int per_row = ldo / V;
  const int c = (int)(e % per_row) * V;
  const long long r = e / per_row;                   // (b*N + n)*k + j
  const int j = (int)(r % k);
  const long long pn = r / k;                        // b*N + n
  float* o = out + (size_t)r * ldo + c;
  if (c >= C) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(o) = make_float4(0.f, 0.f, 0.f, 0.f);
    else o[0] = 0.f;
    return;
  }
  int q = idx[(size_t)pn * idx_ld + j];
  q = q < 0 ? 0 : (q >= N ? N - 1 : q);              // an index outside the cloud is clamped into it: never an out-of-bounds read
  const long long b = pn / N;
  const float* xn = X + ((size_t)b * N + q) * C + c;
  const float* xc = X + (size_t)pn * C + c;
  if constexpr (V == 4) {
    const float4 n4 = *reinterpret_cast<const float4*>(xn), c4 = *reinterpret_cast<const float4*>(xc);
    *reinterpret_cast<float4*>(o) = make_float4(n4.x - c4.x, n4.y - c4.y, n4.z - c4.z, n4.w - c4.w);
  } else {
    o[0] = xn[0] - xc[0];
  }
}

}  // namespace
}  // namespace houv

extern "C" int houv_idam_simmat(const float* src, const float* tgt, const float* es, const float* et, int B, int Ms, int Mt,
                                int E, const float* W1, const float* s1, const float* t1, const float* W2, const float* b2,
                                const float* W3, const float* s3, const float* t3, const float* w4, const float* b4,
                                float* rowmax, int32_t* corr_idx, float* corr, float* scores, void* stream) {
  using namespace houv;
  if (B < 0 || Ms < 1 || Mt < 1) {
    set_error("houv_idam_simmat: bad shape B=%d Ms=%d Mt=%d (Ms, Mt >= 1)", B, Ms, Mt);
    return 0;
  }
  if (E < 4 || E > kSimMaxE || (E & 3)) {
    set_error("houv_idam_simmat: E=%d must be a multiple of 4 in 4..%d", E, kSimMaxE);
    return 0;
  }
  const long long tiles = (Ms + kSimRows - 1) / kSimRows;
  if ((long long)B * tiles > 0x7fffffffLL) {
    set_error("houv_idam_simmat: B=%d x Ms=%d is too many row tiles", B, Ms);
    return 0;
  }
  if (B == 0) return 1;
  if (!src || !tgt || !es || !et || !W1 || !s1 || !t1 || !W2 || !b2 || !W3 || !s3 || !t3 || !w4 || !b4) {
    set_error("houv_idam_simmat: null input pointer");
    return 0;
  }
  if ((reinterpret_cast<uintptr_t>(es) | reinterpret_cast<uintptr_t>(et)) & 15) {
    set_error("houv_idam_simmat: es and et must be 16-byte aligned");
    return 0;
  }
  const SimShape shape{Ms, Mt, E, (int)tiles};
  idam_simmat_kernel<<<(unsigned)(B * tiles), kSimBlock, 0, (hipStream_t)stream>>>(src, tgt, es, et, W1, s1, t1, W2, b2, W3, s3, t3, w4,
                                                                                  b4, rowmax, corr_idx, corr, scores, shape);
  return check_launch("houv_idam_simmat") ? 1 : 0;
}

extern "C" int houv_edge_diff(const float* X, const int32_t* idx, int B, int N, int k, int C, int idx_ld, int ldo, float* out,
                              void* stream) {
  using namespace houv;
  if (B < 0 || N <= 0 || k <= 0 || C <= 0 || (long long)B * N > 0x7fffffffLL) {
    set_error("houv_edge_diff: bad shape B=%d N=%d k=%d C=%d", B, N, k, C);
    return 0;
  }
  if (idx_ld < k || ldo < C) {
    set_error("houv_edge_diff: idx_ld=%d < k=%d or ldo=%d < C=%d", idx_ld, k, ldo, C);
    return 0;
  }
  if (B == 0) return 1;
  if (!X || !idx || !out) {
    set_error("houv_edge_diff: null pointer");
    return 0;
  }
  const bool vec = !(C & 3) && !(ldo & 3) && !((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(out)) & 15);
  const long long total = (long long)B * N * k * (vec ? ldo / 4 : ldo);
  const long long blocks = (total + kEdgeBlock - 1) / kEdgeBlock;
  if (blocks > 0x7fffffffLL) {
    set_error("houv_edge_diff: B=%d N=%d k=%d ldo=%d is too large for one launch", B, N, k, ldo);
    return 0;
  }
  if (vec) edge_diff_kernel<4><<<(unsigned)blocks, kEdgeBlock, 0, (hipStream_t)stream>>>(X, idx, total, N, k, C, idx_ld, ldo, out);
  else edge_diff_kernel<1><<<(unsigned)blocks, kEdgeBlock, 0, (hipStream_t)stream>>>(X, idx, total, N, k, C, idx_ld, ldo, out);
  return check_launch("houv_edge_diff") ? 1 : 0;
}
