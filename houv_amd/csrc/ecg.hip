// ecg.hip -- the two device pieces of the ECG completion network (completion/models/ecg.py):
//
//   houv_knn_feat     k nearest neighbours between C-channel feature rows (get_graph_feature, model_utils.py).  One lane per
//                     query, one wave per workgroup.  Candidates are walked in blocks of 32 whose partial sums live in
//                     registers; channels are walked in chunks of 16 (then 8, 4, 2, 1 for the remainder), so C = 256 needs no
//                     more registers than C = 48.  A candidate's features sit at a wave-uniform address: they arrive through the
//                     scalar cache and enter the vector ALU as scalar operands (one subtract and one fma per pair and channel).
//                     After the last channel the 32 sums pass through LDS ([candidate][lane], a wave-private 8 KB) into the
//                     queued stable insertion of knn_cross_queued_kernel (a 4 KB queue).  The [B, N, N] matrix of the reference never exists.
//   houv_dense_conv   Dense_conv.forward (ecg.py:58-65) in one kernel: lane = point, the k edges in a loop, the three 24-wide
//                     layers as fma chains whose weights sit in LDS and are read at wave-uniform addresses, the maximum over
//                     the neighbours in registers.  Only out[B, N, C + 72] is written.
//
// No atomics, no allocation, no scratch, fixed orders everywhere: results are bit-identical from call to call.
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// feature-space k-NN
// ------------------------------------------------------------------------------------------------------------------
constexpr int kFeatJB = HOUV_KNN_FEAT_BLOCK;     // candidates per block (partial sums in registers)
constexpr int kFeatCC = HOUV_KNN_FEAT_CHUNK;     // channels per full chunk
constexpr int kFeatQueue = 8;                    // queued candidates per lane between two flushes
static_assert(kFeatJB == 32 && kFeatCC == 16, "the remainder ladder below is written for chunks of 16");

// d[j] = fma(t, t, d[j]) for the CC channels from c0 on, c ascending, t = cand[j][c] - q[c]; `cand` is wave-uniform
template <int CC>
__device__ __forceinline__ void feat_accumulate(const float* __restrict__ cand, const float* __restrict__ qrow, int ldx, int c0,
                                                float (&d)[kFeatJB]) {
  float q[CC];
#pragma unroll
  for (int c = 0; c < CC; ++c) q[c] = qrow[c0 + c];
  // four rows' scalar loads are in flight before the first of them is used: with one or two waves on a SIMD nothing else
  // hides their latency
  constexpr int JU = 4;
#pragma unroll
  for (int j = 0; j < kFeatJB; j += JU) {
    float r[JU][CC];
#pragma unroll
    for (int u = 0; u < JU; ++u)
#pragma unroll
      for (int c = 0; c < CC; ++c) r[u][c] = cand[(size_t)(j + u) * ldx + c0 + c];
#pragma unroll
    for (int c = 0; c < CC; ++c) {
#pragma unroll
      for (int u = 0; u < JU; ++u) {
        const float t = r[u][c] - q[c];
        d[j + u] = __builtin_fmaf(t, t, d[j + u]);
      }
    }
  }
}

template <int K>
__global__ __launch_bounds__(kWave) void knn_feat_kernel(const float* __restrict__ x, int N, int C, int ldx, int kout,
                                                         int* __restrict__ idx, float* __restrict__ dist2) {
  __shared__ float s_d[kFeatJB][kWave];
  __shared__ float2 s_q[kFeatQueue][kWave];   // [slot][lane]: (distance, index bits)
  const int b = blockIdx.y, lane = threadIdx.x;
  const int qi = blockIdx.x * kWave + lane;
  const bool ok = qi < N;
  const float* __restrict__ xb = x + (size_t)b * N * ldx;
  const float* __restrict__ qrow = xb + (size_t)min(qi, N - 1) * ldx;   // lanes past the cloud repeat its last row; never stored
  float bd[K];
  int bi[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { bd[j] = INFINITY; bi[j] = 0; }
  // Queued insertions, as in knn_cross_queued_kernel (pointops.hip): a wave runs the insertion bubble for all 64 lanes whenever
  // one lane needs it, so a lane only queues its candidates (in index order) and the queues are flushed in bulk.  The
  // insertion is the stable one: a candidate enters at the first slot it is strictly nearer than, and from there on every
  // entry moves down one slot, equal distances included.
  int qn = 0;                 // entries in this lane's queue
  float thr = INFINITY;       // bd[K-1] as of the last flush
  auto flush = [&]() {
#pragma unroll 1
    for (int s = 0; s < kFeatQueue; ++s) {
      if (!__any(s < qn)) break;
      const float2 e = s_q[s][lane];
      float d = s < qn ? e.x : INFINITY;
      int id = __float_as_int(e.y);
      bool lt = false;
#pragma unroll
      for (int t = 0; t < K; ++t) {
        lt = lt || d < bd[t];
        const float td = bd[t]; const int ti = bi[t];
        bd[t] = lt ? d : td;  bi[t] = lt ? id : ti;
        d = lt ? td : d;      id = lt ? ti : id;
      }
    }
    qn = 0;
    thr = bd[K - 1];
  };
  for (int j0 = 0; j0 < N; j0 += kFeatJB) {
    const int cnt = min(kFeatJB, N - j0);
    // a partial last block is moved back so that all 32 rows exist; the rows it repeats are skipped at insertion
    const int base = max(0, min(j0, N - kFeatJB));
    if (N >= kFeatJB) {
      const float* __restrict__ cand = xb + (size_t)base * ldx;
      float d[kFeatJB];
#pragma unroll
      for (int j = 0; j < kFeatJB; ++j) d[j] = 0.f;
      int c0 = 0;
      for (; c0 + kFeatCC <= C; c0 += kFeatCC) feat_accumulate<kFeatCC>(cand, qrow, ldx, c0, d);
      if ((C - c0) & 8) { feat_accumulate<8>(cand, qrow, ldx, c0, d); c0 += 8; }
      if ((C - c0) & 4) { feat_accumulate<4>(cand, qrow, ldx, c0, d); c0 += 4; }
      if ((C - c0) & 2) { feat_accumulate<2>(cand, qrow, ldx, c0, d); c0 += 2; }
      if ((C - c0) & 1) { feat_accumulate<1>(cand, qrow, ldx, c0, d); }
#pragma unroll
      for (int j = 0; j < kFeatJB; ++j) s_d[j][lane] = d[j];
    } else {
      // clouds of fewer than 32 points: one candidate at a time, the same chain
      for (int j = 0; j < cnt; ++j) {
        const float* __restrict__ r = xb + (size_t)j * ldx;
        float d = 0.f;
        for (int c = 0; c < C; ++c) {
          const float t = r[c] - qrow[c];
          d = __builtin_fmaf(t, t, d);
        }
        s_d[j][lane] = d;
      }
    }
    // queue the block's candidates that pass the (stale, hence conservative) threshold; flush when a lane's queue is full
    const int skip = j0 - base;
    for (int j = 0; j < cnt; ++j) {
      const float d = s_d[skip + j][lane];
      if (d < thr) {
        s_q[qn][lane] = make_float2(d, __int_as_float(j0 + j));
        ++qn;
      }
      if (__any(qn == kFeatQueue)) flush();
    }
  }
  flush();
  if (ok) {
    const size_t o = ((size_t)b * N + qi) * kout;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j < kout) {
        idx[o + j] = bi[j];
        if (dist2) dist2[o + j] = bd[j];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Dense_conv: edge features, three 24-wide layers, maximum over the neighbours
// ------------------------------------------------------------------------------------------------------------------
constexpr int kG = HOUV_DENSE_CONV_GROWTH;
constexpr int kDenseNT = 128;                    // two waves share one LDS copy of the weights

// Weights are read at wave-uniform LDS addresses (broadcasts), four at a time.  Through the scalar cache instead they would
// have to be re-read for every edge (hoisted out of the loop they occupy ~3000 scalar registers), and at 16 to 25 KB per
// pass they evict each other from the 16 KB cache: measured, that kernel spent its time waiting for them.
template <int C>
__global__ __launch_bounds__(kDenseNT) void dense_conv_kernel(const float* __restrict__ x, int ldx, const int* __restrict__ idx,
                                                              int N, int k, const float* __restrict__ W0,
                                                              const float* __restrict__ b0, const float* __restrict__ W1,
                                                              const float* __restrict__ b1, const float* __restrict__ W2,
                                                              const float* __restrict__ b2, int relu_out,
                                                              float* __restrict__ out, int ldo) {
  constexpr int L0 = 2 * C, L1 = kG + C, L2 = 2 * kG + C;      // row lengths of W0, W1, W2: multiples of 4
  __shared__ __attribute__((aligned(16))) float W0s[kG * L0];
  __shared__ __attribute__((aligned(16))) float W1s[kG * L1];
  __shared__ __attribute__((aligned(16))) float W2s[kG * L2];
  __shared__ float bs[3][kG];
  const int b = blockIdx.y, tid = threadIdx.x;
  for (int e = tid; e < kG * L0; e += kDenseNT) W0s[e] = W0[e];
  for (int e = tid; e < kG * L1; e += kDenseNT) W1s[e] = W1[e];
  for (int e = tid; e < kG * L2; e += kDenseNT) W2s[e] = W2[e];
  if (tid < kG) { bs[0][tid] = b0[tid]; bs[1][tid] = b1[tid]; bs[2][tid] = b2[tid]; }
  __syncthreads();

  const int pi = blockIdx.x * kDenseNT + tid;
  const bool ok = pi < N;
  const int i = min(pi, N - 1);                                 // lanes past the cloud repeat its last point; never stored
  const float* __restrict__ xb = x + (size_t)b * N * ldx;
  const int* __restrict__ nb = idx + ((size_t)b * N + i) * k;

  float xi[C];
#pragma unroll
  for (int c = 0; c < C; ++c) xi[c] = xb[(size_t)i * ldx + c];

  // the centre's share of each layer, once per point: the head of W0's chain (its columns come first in cat(x_i, x_j - x_i))
  // and the x_i columns of W1 and W2 with the bias
  float pre0[kG], q1[kG], q2[kG];
#pragma unroll
  for (int o = 0; o < kG; ++o) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      a0 = __builtin_fmaf(W0s[o * L0 + c], xi[c], a0);
      a1 = __builtin_fmaf(W1s[o * L1 + kG + c], xi[c], a1);
      a2 = __builtin_fmaf(W2s[o * L2 + kG + c], xi[c], a2);
    }
    pre0[o] = a0;
    q1[o] = a1 + bs[1][o];
    q2[o] = a2 + bs[2][o];
  }

  float m0[kG], m1[kG], m2[kG];
#pragma unroll
  for (int o = 0; o < kG; ++o) m0[o] = m1[o] = m2[o] = -__builtin_inff();

#pragma unroll 1
  for (int e = 0; e < k; ++e) {
    // an offset of 0 the compiler cannot see through: the weights are re-read from LDS for every edge.  (Hoisted out of the
    // loop, being invariant, they would need ~6000 registers.)
    int z = 0;
    asm volatile("" : "+s"(z));
    const float* __restrict__ W0e = W0s + z;
    const float* __restrict__ W1e = W1s + z;
    const float* __restrict__ W2e = W2s + z;
    const int j = min(max(nb[e], 0), N - 1);
    const float* __restrict__ xj = xb + (size_t)j * ldx;
    float y0[kG], s1[kG];
#pragma unroll
    for (int o = 0; o < kG; ++o) y0[o] = pre0[o];
#pragma unroll
    for (int c4 = 0; c4 < C; c4 += 4) {
      float t[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) t[c] = xj[c4 + c] - xi[c4 + c];
#pragma unroll
      for (int o = 0; o < kG; ++o)
#pragma unroll
        for (int c = 0; c < 4; ++c) y0[o] = __builtin_fmaf(W0e[o * L0 + C + c4 + c], t[c], y0[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      y0[o] = __builtin_fmaxf(y0[o] + bs[0][o], 0.f);
      m0[o] = __builtin_fmaxf(m0[o], y0[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      float a = 0.f;
#pragma unroll
      for (int c = 0; c < kG; ++c) a = __builtin_fmaf(W1e[o * L1 + c], y0[c], a);
      s1[o] = __builtin_fmaxf(a + q1[o], 0.f);
      m1[o] = __builtin_fmaxf(m1[o], s1[o]);
    }
#pragma unroll
    for (int o = 0; o < kG; ++o) {
      float a = 0.f, c2 = 0.f;
#pragma unroll
      for (int c = 0; c < kG; ++c) a = __builtin_fmaf(W2e[o * L2 + c], y0[c], a);
#pragma unroll
      for (int c = 0; c < kG; ++c) c2 = __builtin_fmaf(W2e[o * L2 + kG + C + c], s1[c], c2);
      m2[o] = __builtin_fmaxf(m2[o], (a + q2[o]) + c2);
    }
  }

  if (ok) {
    float* __restrict__ o_ = out + ((size_t)b * N + pi) * ldo;
#pragma unroll
    for (int o = 0; o < kG; ++o) o_[o] = relu_out ? __builtin_fmaxf(m0[o], 0.f) : m0[o];
#pragma unroll
    for (int c = 0; c < C; ++c) o_[kG + c] = relu_out ? __builtin_fmaxf(xi[c], 0.f) : xi[c];
#pragma unroll
    for (int o = 0; o < kG; ++o) o_[kG + C + o] = relu_out ? __builtin_fmaxf(m1[o], 0.f) : m1[o];
#pragma unroll
    for (int o = 0; o < kG; ++o) o_[2 * kG + C + o] = relu_out ? __builtin_fmaxf(m2[o], 0.f) : m2[o];
  }
}

}  // namespace
}  // namespace houv

extern "C" int houv_knn_feat(const float* x, int B, int N, int C, int ldx, int k, int32_t* idx, float* dist2_or_null,
                             void* stream) {
  using namespace houv;
  if (B < 0 || B > 65535 || N < 1 || N > 16384 || C < 1 || C > 256 || ldx < C || k < 1 || k > 32 || k > N) {
    set_error("houv_knn_feat: bad argument B=%d N=%d C=%d ldx=%d k=%d (1 <= C <= 256, ldx >= C, 1 <= k <= 32, k <= N <= 16384, "
              "B <= 65535)", B, N, C, ldx, k);
    return 0;
  }
  if (B == 0) return 1;
  if (!x || !idx) { set_error("houv_knn_feat: null pointer"); return 0; }
  dim3 grid((N + kWave - 1) / kWave, B);
  hipStream_t s = (hipStream_t)stream;
  // the next list size up (4, 16, 32); its first k entries are the k-list
  if (k <= 4) knn_feat_kernel<4><<<grid, kWave, 0, s>>>(x, N, C, ldx, k, idx, dist2_or_null);
  else if (k <= 16) knn_feat_kernel<16><<<grid, kWave, 0, s>>>(x, N, C, ldx, k, idx, dist2_or_null);
  else knn_feat_kernel<32><<<grid, kWave, 0, s>>>(x, N, C, ldx, k, idx, dist2_or_null);
  return check_launch("houv_knn_feat") ? 1 : 0;
}

extern "C" int houv_dense_conv(const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k, const float* W0,
                               const float* b0, const float* W1, const float* b1, const float* W2, const float* b2,
                               int relu_out, float* out, int ldo, void* stream) {
  using namespace houv;
  if (C != 24 && C != 48) {
    set_error("houv_dense_conv: C=%d has no kernel: 24 and 48 are served", C);
    return 0;
  }
  if (k < 1 || k > 32) {
    set_error("houv_dense_conv: k=%d neighbours per point: 1..32 are served", k);
    return 0;
  }
  if (B < 0 || B > 65535 || N < 1 || ldx < C || ldo < C + 3 * kG) {
    set_error("houv_dense_conv: bad argument B=%d N=%d ldx=%d ldo=%d (0 <= B <= 65535, N >= 1, ldx >= C=%d, ldo >= C + 72 = %d)",
              B, N, ldx, ldo, C, C + 3 * kG);
    return 0;
  }
  if (B == 0) return 1;
  {
    const void* req[] = {x, idx, W0, b0, W1, b1, W2, b2, out};
    const char* names[] = {"x", "idx", "W0", "b0", "W1", "b1", "W2", "b2", "out"};
    for (int i = 0; i < 9; ++i)
      if (!req[i]) {
        set_error("houv_dense_conv: %s is a null pointer", names[i]);
        return 0;
      }
  }
  dim3 grid((N + kDenseNT - 1) / kDenseNT, B);
  hipStream_t s = (hipStream_t)stream;
  if (C == 24) dense_conv_kernel<24><<<grid, kDenseNT, 0, s>>>(x, ldx, idx, N, k, W0, b0, W1, b1, W2, b2, relu_out, out, ldo);
  else dense_conv_kernel<48><<<grid, kDenseNT, 0, s>>>(x, ldx, idx, N, k, W0, b0, W1, b1, W2, b2, relu_out, out, ldo);
  return check_launch("houv_dense_conv") ? 1 : 0;
}
