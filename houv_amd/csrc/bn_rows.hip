// bn_rows.hip -- training-mode BatchNorm over point-major rows z[R, C] (row stride ld >= C), the piece every registration head needs
// to train:
//
//   houv_bn_rows_stats           batch mean and biased variance per column
//   houv_bn_relu_rows            y = relu?((z - mean) * rstd * weight + bias), optionally with the column maximum and arg-max of
//                                every group of N_group rows (a cloud's max-pool) from the same read
//   houv_bn_relu_rows_backward   gz, gweight, gbias; the ReLU mask and xhat are recomputed from z
//
// All three stream the rows once or twice and are bound by memory.  A workgroup of 256 lanes is a TX x TY tile: TX lanes side by
// side over the columns, VEC = 4 columns (one 16-byte load) per lane where C, ld and the pointers allow it and 1 otherwise, TY rows
// in flight; TX = min(64, the power of two that covers the columns), so a narrow layer (C = 64: TX = 16, TY = 16) still reads
// whole rows with every lane.  grid.x walks the column tiles and grid.y the rows in chunks of kBnChunk = 128, so the chip is full
// when C is small (many row chunks) and when C is large (column tiles too).
//
// No float atomics anywhere.  Sums over rows: a lane adds its rows in ascending order, the TY lanes of a column are added in ty
// order by the tile's first row of lanes, a chunk's result goes to the workspace, and a second launch combines the chunks in chunk
// order.  The partition depends on (R, C) alone -- not on the device, the stream or earlier calls -- so results are bit-identical
// from call to call.  The variance is never E[z^2] - mean^2: a chunk takes its own mean first and then the squared deviations
// about it (its rows are re-read, from L2), and chunks merge as (count, mean, M2) triples.
// Arithmetic is fp32 with fixed expression trees (-ffp-contract=off).
#include <initializer_list>

#include "houv_common.h"

namespace houv {
namespace {

constexpr int kBnBlock = 256;
constexpr int kBnChunk = 128;          // rows per workgroup and per partial

template <int VEC>
__device__ __forceinline__ void bn_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}

template <int VEC>
__device__ __forceinline__ void bn_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

// The tile's geometry.  tx = lane's column group, ty = its row phase; a lane past the last column is idle but meets the barriers.
struct BnTile {
  int tx, ty, TX, TY, c0;
  bool live;
};
template <int VEC>
__device__ __forceinline__ BnTile bn_tile(int TX, int C) {
  BnTile t;
  t.TX = TX;
  t.TY = kBnBlock / TX;
  t.tx = threadIdx.x % TX;
  t.ty = threadIdx.x / TX;
  t.c0 = (blockIdx.x * TX + t.tx) * VEC;
  t.live = t.c0 < C;
  return t;
}

// Sum v over the TY lanes of every column, in ty order; the total comes back in EVERY lane of the column.  sh: kBnBlock * VEC floats.
template <int VEC>
__device__ __forceinline__ void bn_col_sum(float (&v)[VEC], float* sh, const BnTile& t) {
  __syncthreads();                      // the previous use of sh is over
#pragma unroll
  for (int k = 0; k < VEC; ++k) sh[(t.ty * t.TX + t.tx) * VEC + k] = v[k];
  __syncthreads();
  if (t.ty == 0) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float s = sh[t.tx * VEC + k];
      for (int y = 1; y < t.TY; ++y) s += sh[(y * t.TX + t.tx) * VEC + k];
      sh[t.tx * VEC + k] = s;
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < VEC; ++k) v[k] = sh[t.tx * VEC + k];
}

// ------------------------------------------------------------------------------------------------------------------
// statistics
// ------------------------------------------------------------------------------------------------------------------
// ws[chunk][0][C] = the chunk's mean, ws[chunk][1][C] = its M2 (sum of squared deviations about that mean)
template <int VEC>
__global__ __launch_bounds__(kBnBlock) void bn_stats_chunk_kernel(const float* __restrict__ z, int R, int C, size_t ld, int TX,
                                                                  float* __restrict__ ws) {
  __shared__ float sh[kBnBlock * VEC];
  const BnTile t = bn_tile<VEC>(TX, C);
  const int chunk = blockIdx.y;
  const int r0 = chunk * kBnChunk;
  const int r1 = min(R, r0 + kBnChunk);
  float s[VEC], x[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) s[k] = 0.f;
  if (t.live) {
#pragma unroll 4
    for (int r = r0 + t.ty; r < r1; r += t.TY) {
      bn_load<VEC>(z + (size_t)r * ld + t.c0, x);
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] += x[k];
    }
  }
  bn_col_sum<VEC>(s, sh, t);
  const float n = (float)(r1 - r0);
  float m[VEC], q[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { m[k] = s[k] / n; q[k] = 0.f; }
  if (t.live) {
#pragma unroll 4
    for (int r = r0 + t.ty; r < r1; r += t.TY) {
      bn_load<VEC>(z + (size_t)r * ld + t.c0, x);
#pragma unroll
      for (int k = 0; k < VEC; ++k) { const float d = x[k] - m[k]; q[k] += d * d; }
    }
  }
  bn_col_sum<VEC>(q, sh, t);
  if (t.live && t.ty == 0) {
    bn_store<VEC>(ws + ((size_t)chunk * 2 + 0) * C + t.c0, m);
    bn_store<VEC>(ws + ((size_t)chunk * 2 + 1) * C + t.c0, q);
  }
}

// one lane per column: the chunks' (count, mean, M2) merged in chunk order (Chan, Golub, LeVeque)
__global__ __launch_bounds__(kBnBlock) void bn_stats_combine_kernel(const float* __restrict__ ws, int R, int C, int nchunk,
                                                                    float* __restrict__ mean, float* __restrict__ var) {
  const int c = blockIdx.x * kBnBlock + threadIdx.x;
  if (c >= C) return;
  float n = (float)min(R, kBnChunk), m = ws[c], q = ws[(size_t)C + c];
  for (int i = 1; i < nchunk; ++i) {
    const float nb = (float)min(R - i * kBnChunk, kBnChunk);
    const float mb = ws[((size_t)i * 2 + 0) * C + c], qb = ws[((size_t)i * 2 + 1) * C + c];
    const float tot = n + nb, delta = mb - m, frac = nb / tot;
    m = m + delta * frac;
    q = (q + qb) + (delta * delta) * (n * frac);
    n = tot;
  }
  mean[c] = m;
  var[c] = q / (float)R;
}

// ------------------------------------------------------------------------------------------------------------------
// normalise (+ ReLU) (+ group maxima)
// ------------------------------------------------------------------------------------------------------------------
// The expression both directions share, so that the backward's recomputed ReLU mask is the forward's bit for bit.
__device__ __forceinline__ float bn_xhat(float z, float mean, float rstd) { return (z - mean) * rstd; }
__device__ __forceinline__ float bn_affine(float xhat, float w, float b) { return xhat * w + b; }

template <int VEC>
__device__ __forceinline__ void bn_coeffs(const float* mean, const float* var, const float* weight, const float* bias, float eps,
                                          int c0, float (&m)[VEC], float (&rs)[VEC], float (&w)[VEC], float (&b)[VEC]) {
  float v[VEC];
  bn_load<VEC>(mean + c0, m);
  bn_load<VEC>(var + c0, v);
  bn_load<VEC>(weight + c0, w);
  bn_load<VEC>(bias + c0, b);
#pragma unroll
  for (int k = 0; k < VEC; ++k) rs[k] = 1.f / sqrtf(v[k] + eps);
}

// grid.y = group * S + split: the rows [g * Ng + split * kBnChunk, ...) of group g (Ng = R: one group, no maxima wanted).  With
// gmax set, the lane keeps the maximum of its rows and the first row that attains it; the TY lanes of a column are merged by
// (larger value, then lower row); S == 1 writes gmax / garg, S > 1 the partials pmax / parg [group][split][C] for bn_max_combine.
// A NaN never attains a maximum.
template <int VEC>
__global__ __launch_bounds__(kBnBlock) void bn_relu_rows_kernel(const float* __restrict__ z, size_t ld, int C, int Ng, int S, int TX,
                                                                const float* __restrict__ mean, const float* __restrict__ var,
                                                                const float* __restrict__ weight, const float* __restrict__ bias,
                                                                float eps, int relu, float* __restrict__ y, size_t ldy,
                                                                float* __restrict__ omax, int32_t* __restrict__ oarg) {
  __shared__ float shv[kBnBlock * VEC];
  __shared__ int sha[kBnBlock * VEC];
  const BnTile t = bn_tile<VEC>(TX, C);
  const int g = blockIdx.y / S, split = blockIdx.y % S;
  const int r0 = g * Ng + split * kBnChunk;
  const int r1 = min(g * Ng + Ng, r0 + kBnChunk);
  float best[VEC];
  int arg[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { best[k] = -__builtin_inff(); arg[k] = 0x7fffffff; }
  if (t.live) {
    float m[VEC], rs[VEC], w[VEC], b[VEC], x[VEC];
    bn_coeffs<VEC>(mean, var, weight, bias, eps, t.c0, m, rs, w, b);
#pragma unroll 4
    for (int r = r0 + t.ty; r < r1; r += t.TY) {
      bn_load<VEC>(z + (size_t)r * ld + t.c0, x);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float v = bn_affine(bn_xhat(x[k], m[k], rs[k]), w[k], b[k]);
        if (relu) v = v > 0.f ? v : (v == v ? 0.f : v);
        x[k] = v;
        if (v > best[k]) { best[k] = v; arg[k] = r; }
      }
      bn_store<VEC>(y + (size_t)r * ldy + t.c0, x);
    }
  }
  if (omax == nullptr) return;         // uniform over the workgroup
#pragma unroll
  for (int k = 0; k < VEC; ++k) { shv[(t.ty * t.TX + t.tx) * VEC + k] = best[k]; sha[(t.ty * t.TX + t.tx) * VEC + k] = arg[k]; }
  __syncthreads();
  if (t.live && t.ty == 0) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float bv = best[k];
      int ba = arg[k];
      for (int yy = 1; yy < t.TY; ++yy) {
        const float v = shv[(yy * t.TX + t.tx) * VEC + k];
        const int a = sha[(yy * t.TX + t.tx) * VEC + k];
        if (v > bv || (v == bv && a < ba)) { bv = v; ba = a; }
      }
      if (t.c0 + k < C) {
        omax[(size_t)blockIdx.y * C + t.c0 + k] = bv;
        oarg[(size_t)blockIdx.y * C + t.c0 + k] = ba;
      }
    }
  }
}

// one lane per (group, column): the splits' partial maxima in split order = ascending rows, so a strict > keeps the lowest row
__global__ __launch_bounds__(kBnBlock) void bn_max_combine_kernel(const float* __restrict__ pmax, const int32_t* __restrict__ parg,
                                                                  long long total, int C, int S, float* __restrict__ gmax,
                                                                  int32_t* __restrict__ garg) {
  const long long i = (long long)blockIdx.x * kBnBlock + threadIdx.x;
  if (i >= total) return;
  const long long g = i / C;
  const int c = (int)(i % C);
  float bv = pmax[(size_t)g * S * C + c];
  int ba = parg[(size_t)g * S * C + c];
  for (int s = 1; s < S; ++s) {
    const float v = pmax[((size_t)g * S + s) * C + c];
    const int a = parg[((size_t)g * S + s) * C + c];
    if (v > bv || (v == bv && a < ba)) { bv = v; ba = a; }
  }
  gmax[i] = bv;
  garg[i] = ba;
}

// ------------------------------------------------------------------------------------------------------------------
// backward
// ------------------------------------------------------------------------------------------------------------------
// phase 1: ws[chunk][0][C] = sum over the chunk's rows of g, ws[chunk][1][C] = of g * xhat; g = gy * [y > 0]
template <int VEC>
__global__ __launch_bounds__(kBnBlock) void bn_bwd_sums_kernel(const float* __restrict__ gy, size_t ldg, const float* __restrict__ z,
                                                               size_t ld, int R, int C, int TX, const float* __restrict__ mean,
                                                               const float* __restrict__ var, const float* __restrict__ weight,
                                                               const float* __restrict__ bias, float eps, int relu,
                                                               float* __restrict__ ws) {
  __shared__ float sh[kBnBlock * VEC];
  const BnTile t = bn_tile<VEC>(TX, C);
  const int chunk = blockIdx.y;
  const int r0 = chunk * kBnChunk;
  const int r1 = min(R, r0 + kBnChunk);
  float sg[VEC], sx[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { sg[k] = 0.f; sx[k] = 0.f; }
  if (t.live) {
    float m[VEC], rs[VEC], w[VEC], b[VEC], x[VEC], g[VEC];
    bn_coeffs<VEC>(mean, var, weight, bias, eps, t.c0, m, rs, w, b);
#pragma unroll 4
    for (int r = r0 + t.ty; r < r1; r += t.TY) {
      bn_load<VEC>(z + (size_t)r * ld + t.c0, x);
      bn_load<VEC>(gy + (size_t)r * ldg + t.c0, g);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float xh = bn_xhat(x[k], m[k], rs[k]);
        const float gg = (relu && !(bn_affine(xh, w[k], b[k]) > 0.f)) ? 0.f : g[k];
        sg[k] += gg;
        sx[k] += gg * xh;
      }
    }
  }
  bn_col_sum<VEC>(sg, sh, t);
  bn_col_sum<VEC>(sx, sh, t);
  if (t.live && t.ty == 0) {
    bn_store<VEC>(ws + ((size_t)chunk * 2 + 0) * C + t.c0, sg);
    bn_store<VEC>(ws + ((size_t)chunk * 2 + 1) * C + t.c0, sx);
  }
}

// one lane per column: the chunks' sums added in chunk order -> gbias = sum g, gweight = sum g * xhat
__global__ __launch_bounds__(kBnBlock) void bn_bwd_combine_kernel(const float* __restrict__ ws, int C, int nchunk,
                                                                  float* __restrict__ gweight, float* __restrict__ gbias) {
  const int c = blockIdx.x * kBnBlock + threadIdx.x;
  if (c >= C) return;
  float sg = ws[c], sx = ws[(size_t)C + c];
  for (int i = 1; i < nchunk; ++i) {
    sg += ws[((size_t)i * 2 + 0) * C + c];
    sx += ws[((size_t)i * 2 + 1) * C + c];
  }
  gbias[c] = sg;
  gweight[c] = sx;
}

// phase 2: gz = weight * rstd * ((g - mean_R(g)) - xhat * mean_R(g * xhat)).  gy and gz may be the same buffer: a lane reads an
// element before it writes it and nobody else touches it, so neither is __restrict__.
template <int VEC>
__global__ __launch_bounds__(kBnBlock) void bn_bwd_apply_kernel(const float* gy, size_t ldg, const float* __restrict__ z, size_t ld,
                                                                int R, int C, int TX, const float* __restrict__ mean,
                                                                const float* __restrict__ var, const float* __restrict__ weight,
                                                                const float* __restrict__ bias, float eps, int relu,
                                                                const float* __restrict__ gweight, const float* __restrict__ gbias,
                                                                float* gz, size_t ldz) {
  const BnTile t = bn_tile<VEC>(TX, C);
  if (!t.live) return;
  const int r0 = blockIdx.y * kBnChunk;
  const int r1 = min(R, r0 + kBnChunk);
  float m[VEC], rs[VEC], w[VEC], b[VEC], x[VEC], g[VEC], mg[VEC], mx[VEC];
  bn_coeffs<VEC>(mean, var, weight, bias, eps, t.c0, m, rs, w, b);
  bn_load<VEC>(gbias + t.c0, mg);
  bn_load<VEC>(gweight + t.c0, mx);
  const float n = (float)R;
#pragma unroll
  for (int k = 0; k < VEC; ++k) { mg[k] = mg[k] / n; mx[k] = mx[k] / n; }
#pragma unroll 4
  for (int r = r0 + t.ty; r < r1; r += t.TY) {
    bn_load<VEC>(z + (size_t)r * ld + t.c0, x);
    bn_load<VEC>(gy + (size_t)r * ldg + t.c0, g);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float xh = bn_xhat(x[k], m[k], rs[k]);
      const float gg = (relu && !(bn_affine(xh, w[k], b[k]) > 0.f)) ? 0.f : g[k];
      g[k] = (w[k] * rs[k]) * ((gg - mg[k]) - xh * mx[k]);
    }
    bn_store<VEC>(gz + (size_t)r * ldz + t.c0, g);
  }
}

// ---- host side ---------------------------------------------------------------------------------
inline int bn_chunks(long long rows) { return (int)((rows + kBnChunk - 1) / kBnChunk); }

// VEC = 4 where every row of every buffer starts on a 16-byte boundary and holds whole groups of four columns
inline bool bn_vec4(int C, std::initializer_list<long long> lds, std::initializer_list<const void*> ptrs) {
  if (C % 4) return false;
  for (long long l : lds) if (l % 4) return false;
  for (const void* p : ptrs) if (reinterpret_cast<uintptr_t>(p) & 15) return false;
  return true;
}

inline int bn_tx(int C, int vec) {
  const int groups = (C + vec - 1) / vec;
  int tx = 1;
  while (tx < groups && tx < 64) tx <<= 1;
  return tx;
}

inline bool bn_check_shape(const char* fn, long long R, int C, long long min_rows) {
  if (R < min_rows || C < 1 || R > 0x7fffffffLL - 1024) {
    set_error("%s: bad shape R=%lld C=%d (R >= %lld, C >= 1)", fn, R, C, min_rows);
    return false;
  }
  return true;
}

}  // namespace
}  // namespace houv

extern "C" long long houv_bn_rows_workspace_bytes(long long R, int C, int N_group) {
  using namespace houv;
  if (R < 1 || C < 1 || R > 0x7fffffffLL - 1024 || N_group < 0) return 0;
  long long slots = 2LL * bn_chunks(R);                                          // (mean, M2) or (sum g, sum g xhat) per chunk
  if (N_group > 0 && R % N_group == 0) {
    const long long parts = (R / N_group) * bn_chunks(N_group);
    if (2 * parts > slots) slots = 2 * parts;                                    // (max, arg) per (group, split)
  }
  return ((slots * C * 4 + 15) / 16) * 16;
}

extern "C" int houv_bn_rows_stats(const float* z, long long R, int C, long long ld, float* mean, float* var, void* workspace,
                                  long long workspace_bytes, void* stream) {
  using namespace houv;
  const char* fn = "houv_bn_rows_stats";
  if (!bn_check_shape(fn, R, C, 2)) return 0;
  if (ld < C) {
    set_error("%s: ld=%lld < C=%d", fn, ld, C);
    return 0;
  }
  if (!z || !mean || !var || !workspace) {
    set_error("%s: null pointer", fn);
    return 0;
  }
  if (workspace_bytes < houv_bn_rows_workspace_bytes(R, C, 0) || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_bn_rows_workspace_bytes)", fn,
              workspace_bytes, workspace, houv_bn_rows_workspace_bytes(R, C, 0));
    return 0;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int nchunk = bn_chunks(R);
  const bool v4 = bn_vec4(C, {ld}, {z});
  const int vec = v4 ? 4 : 1, TX = bn_tx(C, vec);
  const dim3 grid((unsigned)(((C + vec - 1) / vec + TX - 1) / TX), (unsigned)nchunk);
  if (grid.y > 65535u) {
    set_error("%s: R=%lld needs more row chunks than a launch takes", fn, R);
    return 0;
  }
  if (v4) bn_stats_chunk_kernel<4><<<grid, kBnBlock, 0, s>>>(z, (int)R, C, (size_t)ld, TX, ws);
  else bn_stats_chunk_kernel<1><<<grid, kBnBlock, 0, s>>>(z, (int)R, C, (size_t)ld, TX, ws);
  bn_stats_combine_kernel<<<(C + kBnBlock - 1) / kBnBlock, kBnBlock, 0, s>>>(ws, (int)R, C, nchunk, mean, var);
  return check_launch(fn) ? 1 : 0;
}

extern "C" int houv_bn_relu_rows(const float* z, long long R, int C, long long ld, const float* mean, const float* var,
                                 const float* weight, const float* bias, float eps, int relu, int N_group, float* y, long long ldy,
                                 float* gmax, int32_t* garg, void* workspace, long long workspace_bytes, void* stream) {
  using namespace houv;
  const char* fn = "houv_bn_relu_rows";
  if (!bn_check_shape(fn, R, C, 1)) return 0;
  if (ld < C || ldy < C) {
    set_error("%s: ld=%lld / ldy=%lld < C=%d", fn, ld, ldy, C);
    return 0;
  }
  if (N_group < 0 || (N_group > 0 && R % N_group != 0)) {
    set_error("%s: N_group=%d does not divide R=%lld", fn, N_group, R);
    return 0;
  }
  if (!z || !mean || !var || !weight || !bias || !y || (N_group > 0 && (!gmax || !garg))) {
    set_error("%s: null pointer", fn);
    return 0;
  }
  hipStream_t s = (hipStream_t)stream;
  const int Ng = N_group > 0 ? N_group : (int)R;
  const long long G = R / Ng;
  const int S = bn_chunks(Ng);
  const bool v4 = bn_vec4(C, {ld, ldy}, {z, y, mean, var, weight, bias});
  const int vec = v4 ? 4 : 1, TX = bn_tx(C, vec);
  if (G * S > 65535LL) {
    set_error("%s: R=%lld in groups of %d needs more workgroups than a launch takes", fn, R, Ng);
    return 0;
  }
  float* omax = nullptr;
  int32_t* oarg = nullptr;
  if (N_group > 0) {
    if (S == 1) {
      omax = gmax;
      oarg = garg;
    } else {
      const long long need = houv_bn_rows_workspace_bytes(R, C, N_group);
      if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
        set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_bn_rows_workspace_bytes)", fn,
                  workspace_bytes, workspace, need);
        return 0;
      }
      omax = (float*)workspace;
      oarg = (int32_t*)workspace + (size_t)G * S * C;
    }
  }
  const dim3 grid((unsigned)(((C + vec - 1) / vec + TX - 1) / TX), (unsigned)(G * S));
  if (v4) bn_relu_rows_kernel<4><<<grid, kBnBlock, 0, s>>>(z, (size_t)ld, C, Ng, S, TX, mean, var, weight, bias, eps, relu, y, (size_t)ldy, omax, oarg);
  else bn_relu_rows_kernel<1><<<grid, kBnBlock, 0, s>>>(z, (size_t)ld, C, Ng, S, TX, mean, var, weight, bias, eps, relu, y, (size_t)ldy, omax, oarg);
  if (N_group > 0 && S > 1) {
    const long long total = G * C;
    bn_max_combine_kernel<<<(unsigned)((total + kBnBlock - 1) / kBnBlock), kBnBlock, 0, s>>>(omax, oarg, total, C, S, gmax, garg);
  }
  return check_launch(fn) ? 1 : 0;
}

extern "C" int houv_bn_relu_rows_backward(const float* gy, long long ldg, const float* z, long long R, int C, long long ld,
                                          const float* mean, const float* var, const float* weight, const float* bias, float eps,
                                          int relu, float* gz, long long ldz, float* gweight, float* gbias, void* workspace,
                                          long long workspace_bytes, void* stream) {
  using namespace houv;
  const char* fn = "houv_bn_relu_rows_backward";
  if (!bn_check_shape(fn, R, C, 1)) return 0;
  if (ld < C || ldg < C || ldz < C) {
    set_error("%s: ld=%lld / ldg=%lld / ldz=%lld < C=%d", fn, ld, ldg, ldz, C);
    return 0;
  }
  if (!gy || !z || !mean || !var || !weight || !bias || !gz || !gweight || !gbias || !workspace) {
    set_error("%s: null pointer", fn);
    return 0;
  }
  const long long need = houv_bn_rows_workspace_bytes(R, C, 0);
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15)) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_bn_rows_workspace_bytes)", fn,
              workspace_bytes, workspace, need);
    return 0;
  }
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int nchunk = bn_chunks(R);
  const bool v4 = bn_vec4(C, {ld, ldg, ldz}, {gy, z, gz, mean, var, weight, bias, gweight, gbias});
  const int vec = v4 ? 4 : 1, TX = bn_tx(C, vec);
  const dim3 grid((unsigned)(((C + vec - 1) / vec + TX - 1) / TX), (unsigned)nchunk);
  if (grid.y > 65535u) {
    set_error("%s: R=%lld needs more row chunks than a launch takes", fn, R);
    return 0;
  }
  if (v4) {
    bn_bwd_sums_kernel<4><<<grid, kBnBlock, 0, s>>>(gy, (size_t)ldg, z, (size_t)ld, (int)R, C, TX, mean, var, weight, bias, eps, relu, ws);
    bn_bwd_combine_kernel<<<(C + kBnBlock - 1) / kBnBlock, kBnBlock, 0, s>>>(ws, C, nchunk, gweight, gbias);
    bn_bwd_apply_kernel<4><<<grid, kBnBlock, 0, s>>>(gy, (size_t)ldg, z, (size_t)ld, (int)R, C, TX, mean, var, weight, bias, eps, relu, gweight, gbias, gz, (size_t)ldz);
  } else {
    bn_bwd_sums_kernel<1><<<grid, kBnBlock, 0, s>>>(gy, (size_t)ldg, z, (size_t)ld, (int)R, C, TX, mean, var, weight, bias, eps, relu, ws);
    bn_bwd_combine_kernel<<<(C + kBnBlock - 1) / kBnBlock, kBnBlock, 0, s>>>(ws, C, nchunk, gweight, gbias);
    bn_bwd_apply_kernel<1><<<grid, kBnBlock, 0, s>>>(gy, (size_t)ldg, z, (size_t)ld, (int)R, C, TX, mean, var, weight, bias, eps, relu, gweight, gbias, gz, (size_t)ldz);
  }
  return check_launch(fn) ? 1 : 0;
}
