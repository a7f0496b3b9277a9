// ef_expand.hip -- EF_expansion (completion/model_utils.py:24-55) past its per-point projections, and its backward (DESIGN.md
// section 9.16).  With proj = [U | V | P | Q] per point (U, V: O columns; P, Q: O r columns), m = idx[b,n,j] and s < r:
//
//   houv_ef_expand            h1 = U_n + V_m;  t_s = W2a_s relu(h1) + P_n[s] + Q_m[s];  e_j[s] = W3 relu(t_s) + b3
//                             out[b, n r + s, :] = max over j of e_j[s], with the slot of each maximum when the caller asks for it.
//   houv_ef_expand_backward   the forward recomputed per (point, slot) from proj; gh1 and gt of every edge go to the workspace, a
//                             gather sums them per point (U, P: over the point's slots; V, Q: over the CSR inverse of the lists),
//                             and the weight sums are chunked houv_gemm_f32 products over workspace rows, added in chunk order.
//
// Tiling: a workgroup of four waves owns 16 consecutive points of one cloud.  The two per-edge products are [16 x O] x [O x O] on
// the fp32-input MFMA (v_mfma_f32_16x16x4_f32): the 16 points are the rows, a wave owns O / 64 column tiles of 16, and both
// operands are read four consecutive k at a time (lane l pairs k = 16 kb + 4 (l / 16) + u with itself in A and B, so the sum is
// complete whatever the order).  The accumulator of lane l holds rows 4 (l / 16) + v, column l % 16 of its tile in every product,
// so the running maximum, the ReLU masks and the slot all stay in that lane's registers.
#include <algorithm>

#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kEfNT = 256;
constexpr int kEfRows = 16;                      // points per workgroup = rows of the MFMA tile
constexpr int kEfMaxN = 16384;
constexpr int kEfMaxK = 8;
constexpr int kEfMaxR = 8;
constexpr int kEfGbChunks = 64;                  // row chunks of the gb3 partials
constexpr int kEfGroupEdges = 32768;             // the backward's workspace holds the edges of one group of whole clouds: about this many
constexpr unsigned kEfMaxBlocks = 65536;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }     // a NaN stays a NaN, as torch.relu has it

// acc += A[16 x O] (LDS rows of stride LD, this lane's row rl) * Wt, where lane l reads Wt's element (k, column) at
// w[k * sk + 0]: `w` already points at this lane's column / row, sk is the stride between consecutive k.
template <int O>
__device__ __forceinline__ f32x4 tile_product(const float* __restrict__ a_row, const float* __restrict__ w, size_t sk, int kh, f32x4 acc) {
#pragma unroll 4
  for (int kb = 0; kb < O; kb += 16) {
    const float4 a = *reinterpret_cast<const float4*>(a_row + kb + 4 * kh);
    const float* __restrict__ wk = w + (size_t)(kb + 4 * kh) * sk;
    const float w0 = wk[0], w1 = wk[sk], w2 = wk[2 * sk], w3 = wk[3 * sk];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, w0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, w1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, w2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, w3, acc, 0, 0, 0);
  }
  return acc;
}

// the clamped lists of the tile's 16 points at slot j, and R = relu(U_n + V_m) in LDS (rows past N repeat row N - 1)
template <int O>
__device__ __forceinline__ void load_edges(const float* __restrict__ pb, int ldp, const int* __restrict__ ib, int N, int k, int n0, int j,
                                           int* __restrict__ ms, float* __restrict__ Rs, float* __restrict__ Rw, size_t e0) {
  constexpr int LD = O + 4;
  const int tid = threadIdx.x;
  if (tid < kEfRows) {
    const int n = min(n0 + tid, N - 1);
    ms[tid] = min(max(ib[(size_t)n * k + j], 0), N - 1);
  }
  __syncthreads();
  for (int e = tid; e < kEfRows * O; e += kEfNT) {
    const int i = e / O, c = e - i * O;
    const int n = min(n0 + i, N - 1);
    const float h = pb[(size_t)n * ldp + c] + pb[(size_t)ms[i] * ldp + O + c];
    const float v = relu_nan(h);
    Rs[i * LD + c] = v;
    if (Rw && n0 + i < N) Rw[(e0 + (size_t)i * k) * O + c] = v == v ? v : 0.f;   // a NaN reaches no maximum: its gt is 0, and so is its term
  }
  __syncthreads();
}

template <int O>
__global__ __launch_bounds__(kEfNT) void ef_expand_kernel(const float* __restrict__ proj, int ldp, const int* __restrict__ idx,
                                                          const float* __restrict__ W2a, int ldw, const float* __restrict__ W3,
                                                          const float* __restrict__ b3, int N, int k, int r, int tiles,
                                                          float* __restrict__ out, int ldo, signed char* __restrict__ arg) {
  constexpr int LD = O + 4, TPW = O / 64;
  __shared__ __attribute__((aligned(16))) float Rs[kEfRows * LD];
  __shared__ __attribute__((aligned(16))) float Hs[kEfRows * LD];
  __shared__ int ms[kEfRows];
  const int b = blockIdx.x / tiles, n0 = (blockIdx.x - b * tiles) * kEfRows, s = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rl = lane & 15, kh = lane >> 4;
  const float* __restrict__ pb = proj + (size_t)b * N * ldp;
  const int* __restrict__ ib = idx + (size_t)b * N * k;
  const int W = 2 * O + 2 * O * r;               // the columns of proj
  float best[TPW][4];
  int ba[TPW][4];
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) best[t][v] = 0.f, ba[t][v] = -1;

  for (int j = 0; j < k; ++j) {
    load_edges<O>(pb, ldp, ib, N, k, n0, j, ms, Rs, nullptr, 0);
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int col = (wave * TPW + t) * 16 + rl;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_product<O>(Rs + rl * LD, W2a + (size_t)(s * O + col) * ldw, 1, kh, acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = 4 * kh + v;
        const int n = min(n0 + i, N - 1);
        const float tt = acc[v] + pb[(size_t)n * ldp + 2 * O + s * O + col] + pb[(size_t)ms[i] * ldp + (W - O * r) + s * O + col];
        Hs[i * LD + col] = relu_nan(tt);
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int col = (wave * TPW + t) * 16 + rl;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_product<O>(Hs + rl * LD, W3 + (size_t)col * O, 1, kh, acc);
      const float bias = b3[col];
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float e = acc[v] + bias;
        if (e == e && (ba[t][v] < 0 || e > best[t][v])) best[t][v] = e, ba[t][v] = j;
      }
    }
    __syncthreads();                             // ms, Rs and Hs are rewritten by the next slot
  }
  const float nan = __builtin_nanf("");
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int col = (wave * TPW + t) * 16 + rl;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int n = n0 + 4 * kh + v;
      if (n >= N) continue;
      const size_t row = ((size_t)b * N + n) * r + s;
      out[row * ldo + col] = ba[t][v] < 0 ? nan : best[t][v];
      if (arg) arg[row * O + col] = (signed char)ba[t][v];
    }
  }
}

// The workspace of the backward, in 4-byte elements.  The clouds are taken in groups of Bg (ef_group) one after the other; the
// workspace holds one group: its E = Bg N k edges in the order (b, n, j), padded to EP = SK KC rows: a group's weight sums run
// over SK chunks of KC edges.
struct EfLayout {
  long long E, EP, KC, SK;
  long long keys, offsets, order, Rw, H2w, gtw, gh1w, gtT, geT, part, gbp, total;
};

inline long long up4(long long n) { return (n + 3) & ~3LL; }

int ef_group(int B, int N, int k) { return std::max(1, std::min(B, kEfGroupEdges / (N * k))); }

EfLayout ef_layout(int B, int N, int O, int k, int r) {             // B: the clouds of one group
  EfLayout l;
  l.E = (long long)B * N * k;
  const long long per = (long long)O * O * (r + 1);                            // one chunk's partials of gW2a and gW3
  const long long want = std::max<long long>(1, std::min<long long>(32, (4LL << 20) / per));
  l.KC = std::max<long long>(32, ((l.E + want - 1) / want + 31) / 32 * 32);
  l.SK = std::max<long long>(1, (l.E + l.KC - 1) / l.KC);
  l.EP = l.SK * l.KC;
  long long o = 0;
  l.keys = o; o += up4(l.E);
  l.offsets = o; o += up4((long long)B * (N + 1));
  l.order = o; o += up4(l.E);
  l.Rw = o; o += l.EP * O;
  l.H2w = o; o += l.EP * O * r;
  l.gtw = o; o += l.EP * O * r;
  l.gh1w = o; o += l.EP * O;
  l.gtT = o; o += l.EP * O * r;
  l.geT = o; o += l.EP * O * r;
  l.part = o; o += l.SK * per;
  l.gbp = o; o += (long long)kEfGbChunks * O;
  l.total = o;
  return l;
}

struct EfWs {
  float *Rw, *H2w, *gtw, *gh1w, *gtT, *geT;
  long long EP;
};

// Workgroup (tile, j): the 16 points' edges at slot j.  Per sub-row s: t_s and its mask, ge_s from g and arg, gh2 = ge_s W3,
// gt_s = gh2 [t_s > 0], gh1 += gt_s W2a_s; then gh1 [h1 > 0].  Everything the sums need goes to the workspace.
template <int O>
__global__ __launch_bounds__(kEfNT) void ef_expand_bw_kernel(const float* __restrict__ proj, int ldp, const int* __restrict__ idx,
                                                             const signed char* __restrict__ arg, const float* __restrict__ W2a, int ldw,
                                                             const float* __restrict__ W3, const float* __restrict__ g, int ldg, int N,
                                                             int k, int r, int tiles, const EfWs ws) {
  constexpr int LD = O + 4, TPW = O / 64;
  __shared__ __attribute__((aligned(16))) float Rs[kEfRows * LD];
  __shared__ __attribute__((aligned(16))) float Gs[kEfRows * LD];
  __shared__ __attribute__((aligned(16))) float Ts[kEfRows * LD];
  __shared__ int ms[kEfRows];
  const int b = blockIdx.x / tiles, n0 = (blockIdx.x - b * tiles) * kEfRows, j = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, rl = lane & 15, kh = lane >> 4;
  const float* __restrict__ pb = proj + (size_t)b * N * ldp;
  const int* __restrict__ ib = idx + (size_t)b * N * k;
  const int W = 2 * O + 2 * O * r, Or = O * r;
  const size_t e0 = ((size_t)b * N + n0) * k + j;                              // edge of row i: e0 + i k
  const size_t EP = (size_t)ws.EP;
  load_edges<O>(pb, ldp, ib, N, k, n0, j, ms, Rs, ws.Rw, e0);
  f32x4 gh1[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) gh1[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int s = 0; s < r; ++s) {
    bool live[TPW][4];                           // t_s > 0
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int col = (wave * TPW + t) * 16 + rl;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_product<O>(Rs + rl * LD, W2a + (size_t)(s * O + col) * ldw, 1, kh, acc);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = 4 * kh + v;
        const int n = min(n0 + i, N - 1);
        const float tt = acc[v] + pb[(size_t)n * ldp + 2 * O + s * O + col] + pb[(size_t)ms[i] * ldp + (W - Or) + s * O + col];
        live[t][v] = tt > 0.f;
        if (n0 + i < N) ws.H2w[(e0 + (size_t)i * k) * Or + s * O + col] = tt > 0.f ? tt : 0.f;
      }
    }
    for (int e = threadIdx.x; e < kEfRows * O; e += kEfNT) {
      const int i = e / O, c = e - i * O;
      const int n = n0 + i;
      float val = 0.f;
      if (n < N) {
        const size_t row = ((size_t)b * N + n) * r + s;
        if (arg[row * O + c] == j) val = g[row * ldg + c];
        ws.geT[(size_t)c * (EP * r) + (e0 + (size_t)i * k) * r + s] = val;
      }
      Gs[i * LD + c] = val;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int col = (wave * TPW + t) * 16 + rl;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = tile_product<O>(Gs + rl * LD, W3 + col, O, kh, acc);               // gh2[i] = sum over c of ge[c] W3[c][i]
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = 4 * kh + v;
        const float gt = live[t][v] ? acc[v] : 0.f;
        Ts[i * LD + col] = gt;
        if (n0 + i < N) {
          const size_t e = e0 + (size_t)i * k;
          ws.gtw[e * Or + s * O + col] = gt;
          ws.gtT[(size_t)(s * O + col) * EP + e] = gt;
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      const int col = (wave * TPW + t) * 16 + rl;
      gh1[t] = tile_product<O>(Ts + rl * LD, W2a + (size_t)s * O * ldw + col, ldw, kh, gh1[t]);      // sum over c of gt[c] W2a_s[c][i]
    }
    __syncthreads();                             // Gs and Ts are rewritten by the next sub-row
  }
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int col = (wave * TPW + t) * 16 + rl;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int i = 4 * kh + v;
      if (n0 + i < N) ws.gh1w[(e0 + (size_t)i * k) * O + col] = Rs[i * LD + col] > 0.f ? gh1[t][v] : 0.f;
    }
  }
}

__global__ __launch_bounds__(kEfNT) void ef_keys_kernel(const int* __restrict__ idx, size_t total, int N, int* __restrict__ keys) {
  for (size_t e = (size_t)blockIdx.x * kEfNT + threadIdx.x; e < total; e += (size_t)gridDim.x * kEfNT)
    keys[e] = min(max(idx[e], 0), N - 1);
}

// rows [E, EP) of the row-major operands and columns [E, EP) of the transposed ones are zero: the chunked products read them
__global__ __launch_bounds__(kEfNT) void ef_pad_kernel(EfWs ws, long long E, int O, int r) {
  const long long pad = ws.EP - E, Or = (long long)O * r;
  const long long nR = pad * O, nH = pad * Or, nT = pad * Or, nG = pad * Or;
  for (long long e = (long long)blockIdx.x * kEfNT + threadIdx.x; e < nR + nH + nT + nG; e += (long long)gridDim.x * kEfNT) {
    if (e < nR) ws.Rw[E * O + e] = 0.f;
    else if (e < nR + nH) ws.H2w[E * Or + (e - nR)] = 0.f;
    else if (e < nR + nH + nT) {
      const long long q = e - nR - nH, row = q / pad;
      ws.gtT[row * ws.EP + E + (q - row * pad)] = 0.f;
    } else {
      const long long q = e - nR - nH - nT, row = q / (pad * r);                // geT rows hold EP r columns
      ws.geT[row * ws.EP * r + E * r + (q - row * pad * r)] = 0.f;
    }
  }
}

// gproj[row] = [ sum_j gh1 | sum over the edges that list the row of gh1 | sum_j gt | the same of gt ], slots and edges ascending
__global__ __launch_bounds__(kEfNT) void ef_gproj_kernel(const float* __restrict__ gh1w, const float* __restrict__ gtw,
                                                         const int* __restrict__ offsets, const int* __restrict__ order, size_t total,
                                                         int N, int O, int k, int r, float* __restrict__ gproj, int ldgp) {
  const int Or = O * r, W = 2 * O + 2 * Or;
  for (size_t e = (size_t)blockIdx.x * kEfNT + threadIdx.x; e < total; e += (size_t)gridDim.x * kEfNT) {
    const size_t row = e / W;                    // b * N + n
    const int c = (int)(e - row * W);
    const size_t b = row / N;
    const int n = (int)(row - b * N);
    const bool wide = c >= 2 * O;                // the P and Q columns read gt
    const float* __restrict__ src = wide ? gtw : gh1w;
    const int w = wide ? Or : O;
    const int cc = wide ? c - 2 * O : c;
    float acc = 0.f;
    if (cc < w) {
      const float* __restrict__ p = src + row * k * w + cc;
      for (int j = 0; j < k; ++j) acc += p[(size_t)j * w];
    } else {
      const int* __restrict__ ord = order + b * (size_t)N * k;
      const float* __restrict__ p = src + b * (size_t)N * k * w + (cc - w);
      const int end = offsets[b * ((size_t)N + 1) + n + 1];
      for (int q = offsets[b * ((size_t)N + 1) + n]; q < end; ++q) acc += p[(size_t)ord[q] * w];
    }
    gproj[row * ldgp + c] = acc;
  }
}

// gb3 partials: workgroup (column group of 64, chunk) sums its rows ascending per lane, the four row lanes in order
__global__ __launch_bounds__(kEfNT) void ef_gb3_kernel(const float* __restrict__ g, int ldg, const signed char* __restrict__ arg,
                                                       long long rows, int O, float* __restrict__ part) {
  __shared__ float red[kEfNT];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6, chunk = blockIdx.y;
  const long long per = (rows + kEfGbChunks - 1) / kEfGbChunks;
  const long long r1 = min(rows, (chunk + 1) * per);
  float acc = 0.f;
  for (long long row = chunk * per + q; row < r1; row += 4)
    if (arg[row * O + c] >= 0) acc += g[row * ldg + c];
  red[threadIdx.x] = acc;
  __syncthreads();
  if (q == 0) part[(size_t)chunk * O + c] = ((red[threadIdx.x] + red[threadIdx.x + 64]) + red[threadIdx.x + 128]) + red[threadIdx.x + 192];
}

// out[i] = (first ? nothing : out[i]) + the sum over s < S of part[s * n + i], one after the other, s ascending
__global__ __launch_bounds__(kEfNT) void ef_fold_kernel(const float* __restrict__ part, int S, long long n, float* __restrict__ out,
                                                        int first) {
  const long long i = (long long)blockIdx.x * kEfNT + threadIdx.x;
  if (i >= n) return;
  float v = first ? part[i] : out[i] + part[i];
  for (int s = 1; s < S; ++s) v += part[(size_t)s * n + i];
  out[i] = v;
}

unsigned ef_grid(size_t total) {
  const size_t blocks = (total + kEfNT - 1) / kEfNT;
  return (unsigned)(blocks > kEfMaxBlocks ? kEfMaxBlocks : (blocks ? blocks : 1));
}

// the shape checks both entry points share; false with the error set
bool ef_shape_ok(const char* fn, int B, int N, int O, int k, int r) {
  if (O != 64 && O != 128 && O != 256) { set_error("%s: O=%d output channels has no kernel: 64, 128 and 256 are served", fn, O); return false; }
  if (r < 1 || r > kEfMaxR) { set_error("%s: r=%d sub-rows per point: 1..%d are served", fn, r, kEfMaxR); return false; }
  if (k < 1 || k > kEfMaxK) { set_error("%s: k=%d neighbours per point: 1..%d are served", fn, k, kEfMaxK); return false; }
  if (N < 1 || N > kEfMaxN) { set_error("%s: N=%d points: 1..%d are served", fn, N, kEfMaxN); return false; }
  if ((long long)N * r * O > 0x7fffffffLL) { set_error("%s: N=%d r=%d O=%d: N * r * O < 2^31 is served", fn, N, r, O); return false; }
  if (B < 0) { set_error("%s: B=%d clouds: B >= 0 is served", fn, B); return false; }
  if ((long long)B * ((N + kEfRows - 1) / kEfRows) > 0x7fffffffLL) { set_error("%s: B=%d x N=%d is too large for one call", fn, B, N); return false; }
  return true;
}

}  // namespace
}  // namespace houv

extern "C" int houv_ef_expand(const float* proj, int ldp, const int32_t* idx, int B, int N, int O, int k, int r, const float* W2a, int ldw,
                              const float* W3, const float* b3, float* out, int ldo, int8_t* arg_or_null, void* stream) {
  using namespace houv;
  const char* fn = "houv_ef_expand";
  if (!ef_shape_ok(fn, B, N, O, k, r)) return 0;
  const int W = 2 * O + 2 * O * r;
  if (ldp < W) { set_error("%s: ldp=%d is less than 2 O + 2 O r = %d", fn, ldp, W); return 0; }
  if (ldw < O) { set_error("%s: ldw=%d is less than O=%d", fn, ldw, O); return 0; }
  if (ldo < O) { set_error("%s: ldo=%d is less than O=%d", fn, ldo, O); return 0; }
  if (B == 0) return 1;
  {
    const void* req[] = {proj, idx, W2a, W3, b3, out};
    const char* names[] = {"proj", "idx", "W2a", "W3", "b3", "out"};
    for (int i = 0; i < 6; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  const int tiles = (N + kEfRows - 1) / kEfRows;
  const dim3 grid((unsigned)(B * tiles), (unsigned)r);
  hipStream_t st = (hipStream_t)stream;
  signed char* arg = reinterpret_cast<signed char*>(arg_or_null);
  if (O == 64) ef_expand_kernel<64><<<grid, kEfNT, 0, st>>>(proj, ldp, idx, W2a, ldw, W3, b3, N, k, r, tiles, out, ldo, arg);
  else if (O == 128) ef_expand_kernel<128><<<grid, kEfNT, 0, st>>>(proj, ldp, idx, W2a, ldw, W3, b3, N, k, r, tiles, out, ldo, arg);
  else ef_expand_kernel<256><<<grid, kEfNT, 0, st>>>(proj, ldp, idx, W2a, ldw, W3, b3, N, k, r, tiles, out, ldo, arg);
  return check_launch(fn) ? 1 : 0;
}

extern "C" long long houv_ef_expand_backward_workspace_bytes(int B, int N, int O, int k, int r) {
  using namespace houv;
  if (B <= 0 || N < 1 || N > kEfMaxN || (O != 64 && O != 128 && O != 256) || k < 1 || k > kEfMaxK || r < 1 || r > kEfMaxR ||
      (long long)N * r * O > 0x7fffffffLL)
    return 0;
  return ef_layout(ef_group(B, N, k), N, O, k, r).total * 4;
}

extern "C" int houv_ef_expand_backward(const float* proj, int ldp, const int32_t* idx, const int8_t* arg, int B, int N, int O, int k,
                                       int r, const float* W2a, int ldw, const float* W3, const float* g, int ldg, float* gproj,
                                       int ldgp, float* gW2a, float* gW3, float* gb3, void* workspace, long long workspace_bytes,
                                       void* stream) {
  using namespace houv;
  const char* fn = "houv_ef_expand_backward";
  if (!ef_shape_ok(fn, B, N, O, k, r)) return 0;
  const int Or = O * r, W = 2 * O + 2 * Or;
  if (ldp < W) { set_error("%s: ldp=%d is less than 2 O + 2 O r = %d", fn, ldp, W); return 0; }
  if (ldw < O) { set_error("%s: ldw=%d is less than O=%d", fn, ldw, O); return 0; }
  if (ldg < O) { set_error("%s: ldg=%d is less than O=%d", fn, ldg, O); return 0; }
  if (ldgp < W) { set_error("%s: ldgp=%d is less than 2 O + 2 O r = %d", fn, ldgp, W); return 0; }
  {
    const void* req[] = {gW2a, gW3, gb3};
    const char* names[] = {"gW2a", "gW3", "gb3"};
    for (int i = 0; i < 3; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  hipStream_t st = (hipStream_t)stream;
  if (B == 0) {                                  // no cloud: the weight gradients are zero
    if (hipMemsetAsync(gW2a, 0, (size_t)Or * O * 4, st) != hipSuccess || hipMemsetAsync(gW3, 0, (size_t)O * O * 4, st) != hipSuccess ||
        hipMemsetAsync(gb3, 0, (size_t)O * 4, st) != hipSuccess) {
      set_error("%s: hipMemsetAsync failed", fn);
      return 0;
    }
    return 1;
  }
  {
    const void* req[] = {proj, idx, arg, W2a, W3, g, gproj};
    const char* names[] = {"proj", "idx", "arg", "W2a", "W3", "g", "gproj"};
    for (int i = 0; i < 7; ++i)
      if (!req[i]) {
        set_error("%s: %s is a null pointer", fn, names[i]);
        return 0;
      }
  }
  const long long need = houv_ef_expand_backward_workspace_bytes(B, N, O, k, r);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 15)) {
    set_error("%s: workspace of %lld bytes at %p, %lld are needed, 16-byte aligned (houv_ef_expand_backward_workspace_bytes)", fn,
              workspace_bytes, workspace, need);
    return 0;
  }
  const int Bg = ef_group(B, N, k);
  const EfLayout l = ef_layout(Bg, N, O, k, r);
  float* wf = static_cast<float*>(workspace);
  int* wi = static_cast<int*>(workspace);
  int *keys = wi + l.keys, *offsets = wi + l.offsets, *order = wi + l.order;
  const EfWs ws{wf + l.Rw, wf + l.H2w, wf + l.gtw, wf + l.gh1w, wf + l.gtT, wf + l.geT, l.EP};
  float *part = wf + l.part, *gbp = wf + l.gbp;
  const int tiles = (N + kEfRows - 1) / kEfRows;
  const long long w2 = (long long)Or * O, w3 = (long long)O * O;
  auto blocks = [](long long n) { return (unsigned)((n + kEfNT - 1) / kEfNT); };

  for (int b0 = 0; b0 < B; b0 += Bg) {           // one group of whole clouds after the other: the list sums stay inside a cloud
    const int nb = std::min(Bg, B - b0);
    const long long E = (long long)nb * N * k;
    const size_t p0 = (size_t)b0 * N;            // the group's first point
    const float* pg = proj + p0 * ldp;
    const int32_t* ig = idx + p0 * k;
    const signed char* ag = reinterpret_cast<const signed char*>(arg) + p0 * r * O;
    const float* gg = g + p0 * r * ldg;
    ef_keys_kernel<<<ef_grid((size_t)E), kEfNT, 0, st>>>(ig, (size_t)E, N, keys);
    if (!check_launch(fn)) return 0;
    if (!scatter_index_launch(keys, nb, N, N * k, offsets, order, st)) return 0;
    if (l.EP > E) {
      ef_pad_kernel<<<ef_grid((size_t)((l.EP - E) * (O + 3LL * Or))), kEfNT, 0, st>>>(ws, E, O, r);
      if (!check_launch(fn)) return 0;
    }
    const dim3 grid((unsigned)(nb * tiles), (unsigned)k);
    if (O == 64) ef_expand_bw_kernel<64><<<grid, kEfNT, 0, st>>>(pg, ldp, ig, ag, W2a, ldw, W3, gg, ldg, N, k, r, tiles, ws);
    else if (O == 128) ef_expand_bw_kernel<128><<<grid, kEfNT, 0, st>>>(pg, ldp, ig, ag, W2a, ldw, W3, gg, ldg, N, k, r, tiles, ws);
    else ef_expand_bw_kernel<256><<<grid, kEfNT, 0, st>>>(pg, ldp, ig, ag, W2a, ldw, W3, gg, ldg, N, k, r, tiles, ws);
    if (!check_launch(fn)) return 0;
    ef_gproj_kernel<<<ef_grid((size_t)nb * N * W), kEfNT, 0, st>>>(ws.gh1w, ws.gtw, offsets, order, (size_t)nb * N * W, N, O, k, r,
                                                                  gproj + p0 * ldgp, ldgp);
    if (!check_launch(fn)) return 0;
    // gW2a[O r, O] += gt^T relu(h1) and gW3[O, O] += ge^T h2 (rows (edge, s)): SK chunks over the GEMM's outer dimension, the
    // partials added to the running sum chunks ascending, groups ascending
    if (!houv_gemm_f32(ws.gtT, ws.Rw, part, Or, O, (int)l.KC, (int)l.EP, O, O, 0, (int)l.SK, 1, l.KC, 0, l.KC * O, 0, w2, 0, 1.f, nullptr,
                       nullptr, nullptr, 0, 0, 0, 0, stream))
      return 0;
    ef_fold_kernel<<<blocks(w2), kEfNT, 0, st>>>(part, (int)l.SK, w2, gW2a, b0 == 0);
    if (!check_launch(fn)) return 0;
    float* part3 = part + l.SK * w2;
    if (!houv_gemm_f32(ws.geT, ws.H2w, part3, O, O, (int)(l.KC * r), (int)(l.EP * r), O, O, 0, (int)l.SK, 1, l.KC * r, 0, l.KC * r * O, 0,
                       w3, 0, 1.f, nullptr, nullptr, nullptr, 0, 0, 0, 0, stream))
      return 0;
    ef_fold_kernel<<<blocks(w3), kEfNT, 0, st>>>(part3, (int)l.SK, w3, gW3, b0 == 0);
    if (!check_launch(fn)) return 0;
  }
  const signed char* a = reinterpret_cast<const signed char*>(arg);
  const dim3 gbgrid((unsigned)(O / 64), (unsigned)kEfGbChunks);
  ef_gb3_kernel<<<gbgrid, kEfNT, 0, st>>>(g, ldg, a, (long long)B * N * r, O, gbp);
  if (!check_launch(fn)) return 0;
  ef_fold_kernel<<<blocks(O), kEfNT, 0, st>>>(gbp, kEfGbChunks, O, gb3, 1);
  return check_launch(fn) ? 1 : 0;
}
