// emd.hip -- the auction-algorithm EMD of utils/metrics/EMD (emd_cuda.cu, emd_module.py), one workgroup and ONE launch per
// cloud for the whole auction, with exact tie rules (contract: include/houv_hip.h `houv_emd_forward`).
//
//   emd_auction_kernel<false>  N <= 4096: objects (x, y, z, price), award keys, owners, assignment and the compact bidder list
//                              live in LDS (36 B per point + 16 B: 144 KiB at 4096 points).
//   emd_auction_kernel<true>   4097..16384 points: price / owner / assignment / bid list / increments in the caller's workspace;
//                              objects stream through LDS in tiles of kEmdTile with their prices; award keys per tile in LDS.
//   emd_backward_kernel        one lane per point: gradxyz1 += 2 g (xyz1 - xyz2[assignment]).
//
// Per iteration: compact the unassigned bidders into a list (ballot + one LDS add per wave) -> bid (each bidder's best object,
// lowest index on ties, and second-best value) -> award (LDS 64-bit atomicMax on (inc bits << 32 | ~i): largest increment,
// lowest bidder on ties) -> evict / assign / raise the price.  The bid and award results do not depend on the order of the list
// or on which lanes evaluate which pairs, so the result is bit-identical to the sequential restatement (tests/emd_host.py).
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kEmdBlock = 1024;     // 16 waves: one workgroup per cloud
constexpr int kEmdTile = 4096;      // objects per LDS tile of the streamed kernel (= the in-LDS kernel's largest cloud)
constexpr int kEmdMaxN = 16384;     // bidder and object indices share one 32-bit list word (16 bits each)

__host__ __device__ inline int emd_stride(int N) { return (N + 3) & ~3; }

// One bidder against one object: v = (3 - |y_j - x_i|) - price_j, fp32, no contraction (-ffp-contract=off), correctly
// rounded sqrtf.  Running (best, lowest j of best, max of the others) over objects visited in increasing j.
__device__ __forceinline__ void emd_visit(const float4 o, int j, float x, float y, float z, float& best, float& second,
                                          int& bj) {
  const float dx = o.x - x, dy = o.y - y, dz = o.z - z;
  const float v = (3.0f - sqrtf((dx * dx + dy * dy) + dz * dz)) - o.w;
  const bool gt = v > best;
  second = gt ? best : (v > second ? v : second);
  best = gt ? v : best;
  bj = gt ? j : bj;
}

// Merge two partial results over disjoint object sets: the larger best (lower j on ties); second = max(other best, seconds).
__device__ __forceinline__ void emd_merge(float& best, float& second, int& bj, float b2, float s2, int j2) {
  const bool take = b2 > best || (b2 == best && j2 < bj);
  const float other = take ? best : b2;
  float s = second > s2 ? second : s2;
  s = s > other ? s : other;
  best = take ? b2 : best;
  bj = take ? j2 : bj;
  second = s;
}

__device__ __forceinline__ unsigned long long emd_key(float inc, int i) {
  return ((unsigned long long)__float_as_uint(inc) << 32) | (unsigned)(0xffffffffu - (unsigned)i);
}

// Device-side view of one cloud's auction state.  STREAM = false: LDS arrays; true: the workspace (price, owner, assign, list,
// inc; emd_stride(N) words each) with objects and keys of ONE tile in LDS.
template <bool STREAM>
struct EmdState {
  float4* obj;                 // [tile] (x, y, z, price) -- the in-LDS kernel keeps the prices here
  unsigned long long* key;     // [tile] award keys
  int* cnt;                    // [2] unassigned counts, alternating by iteration parity
  int* owner;                  // [N]
  int* assign;                 // [N]
  unsigned* list;              // [N] bidder i, after the bid i | j* << 16
  float* price;                // [N] (STREAM only)
  float* inc;                  // [N] (STREAM only) increment of list[k]
};

// Bid phase for the cnt listed bidders: P bidders per lane, each spread over a group of G lanes (a power of two <= 64) that
// split the objects j = r, r + G, ...; the group's partial results merge through shuffles.
template <bool STREAM, int P>
__device__ void emd_bid(const EmdState<STREAM>& st, const float* __restrict__ p1, const float* __restrict__ p2, int N, int cnt,
                        float eps, bool last) {
  const int tid = threadIdx.x;
  int q = (kEmdBlock * P) / cnt;
  q = q < 1 ? 1 : q;
  const int lg = min(6, 31 - __clz(q));
  const int G = 1 << lg, r = tid & (G - 1), g = tid >> lg;
  const int cap = (kEmdBlock >> lg) * P;
  for (int base = 0; base < cnt; base += cap) {
    float x[P], y[P], z[P], best[P], second[P];
    int bj[P], bi[P];
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const int k = base + g * P + p;
      bi[p] = k < cnt ? (int)st.list[k] : -1;
      const int i = bi[p] < 0 ? 0 : bi[p];
      x[p] = p1[i * 3 + 0]; y[p] = p1[i * 3 + 1]; z[p] = p1[i * 3 + 2];
      best[p] = -INFINITY; second[p] = -INFINITY; bj[p] = 0x7fffffff;
    }
    const int tile = STREAM ? kEmdTile : N;
    for (int t0 = 0; t0 < N; t0 += tile) {
      const int tn = min(tile, N - t0);
      if constexpr (STREAM) {
        __syncthreads();                              // previous tile / previous chunk done with st.obj
        for (int j = tid; j < tn; j += kEmdBlock) {
          const int jj = t0 + j;
          st.obj[j] = make_float4(p2[jj * 3 + 0], p2[jj * 3 + 1], p2[jj * 3 + 2], st.price[jj]);
        }
        __syncthreads();
      }
      for (int j = r; j < tn; j += G) {
        const float4 o = st.obj[j];
#pragma unroll
        for (int p = 0; p < P; ++p) emd_visit(o, t0 + j, x[p], y[p], z[p], best[p], second[p], bj[p]);
      }
    }
    for (int o = 1; o < G; o <<= 1) {
#pragma unroll
      for (int p = 0; p < P; ++p) {
        const float b2 = __shfl_xor(best[p], o, kWave), s2 = __shfl_xor(second[p], o, kWave);
        const int j2 = __shfl_xor(bj[p], o, kWave);
        emd_merge(best[p], second[p], bj[p], b2, s2, j2);
      }
    }
    if (r == 0) {
#pragma unroll
      for (int p = 0; p < P; ++p) {
        if (bi[p] < 0) continue;
        const int k = base + g * P + p;
        if (bj[p] >= N) bj[p] = 0;                    // only non-finite values leave it unset: keep every index in range
        const float inc = (best[p] - (N == 1 ? best[p] : second[p])) + eps;
        st.list[k] = (unsigned)bi[p] | ((unsigned)bj[p] << 16);
        if constexpr (STREAM) st.inc[k] = inc;
        else if (!last) atomicMax(&st.key[bj[p]], emd_key(inc, bi[p]));
      }
    }
  }
}

template <bool STREAM>
__global__ __launch_bounds__(kEmdBlock) void emd_auction_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                                int N, float eps, int iters, float* __restrict__ dist,
                                                                int* __restrict__ assignment, int* __restrict__ iters_run,
                                                                unsigned char* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const float* __restrict__ p1 = xyz1 + (size_t)b * N * 3;
  const float* __restrict__ p2 = xyz2 + (size_t)b * N * 3;
  const int Np = emd_stride(N);
  const int tile = STREAM ? kEmdTile : Np;
  EmdState<STREAM> st;
  st.obj = (float4*)smem;
  st.key = (unsigned long long*)(smem + 16 * (size_t)tile);
  st.cnt = (int*)(smem + 24 * (size_t)tile);
  if constexpr (STREAM) {
    unsigned char* w = ws + (size_t)b * 20 * Np;
    st.price = (float*)w;
    st.owner = (int*)(w + 4 * (size_t)Np);
    st.assign = (int*)(w + 8 * (size_t)Np);
    st.list = (unsigned*)(w + 12 * (size_t)Np);
    st.inc = (float*)(w + 16 * (size_t)Np);
    for (int j = tid; j < N; j += kEmdBlock) { st.price[j] = 0.f; st.owner[j] = -1; st.assign[j] = -1; }
  } else {
    st.owner = (int*)(smem + 24 * (size_t)tile + 16);
    st.assign = st.owner + Np;
    st.list = (unsigned*)(st.assign + Np);
    st.price = nullptr;
    st.inc = nullptr;
    for (int j = tid; j < N; j += kEmdBlock) {
      st.obj[j] = make_float4(p2[j * 3 + 0], p2[j * 3 + 1], p2[j * 3 + 2], 0.f);
      st.owner[j] = -1;
      st.assign[j] = -1;
    }
  }
  if (tid < 2) st.cnt[tid] = 0;
  __syncthreads();

  int t = 0;
  for (; t < iters; ++t) {
    const bool last = t == iters - 1;
    int* cntp = st.cnt + (t & 1);
    if (tid == 0) st.cnt[(t + 1) & 1] = 0;            // read for the last time in the previous iteration's bid phase
    // 1. compact U = { i : assign[i] == -1 }: ballot, one LDS add per wave, lane rank by mbcnt (the list order is immaterial)
    for (int i0 = 0; i0 < N; i0 += kEmdBlock) {
      const int i = i0 + tid;
      const bool u = i < N && st.assign[i] == -1;
      const unsigned long long m = __ballot(u);
      if (m != 0ull) {
        int base = 0;
        if (lane == 0) base = atomicAdd(cntp, (int)__popcll(m));
        base = __shfl(base, 0, kWave);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (u) st.list[base + rank] = (unsigned)i;
      }
    }
    if constexpr (!STREAM)
      for (int j = tid; j < N; j += kEmdBlock) st.key[j] = 0ull;   // below every real key: inc >= eps > 0
    __syncthreads();
    const int cnt = *cntp;
    if (cnt == 0) break;                              // every later iteration would change nothing
    // 2. bid
    if (cnt > kEmdBlock) emd_bid<STREAM, 4>(st, p1, p2, N, cnt, eps, last);
    else emd_bid<STREAM, 1>(st, p1, p2, N, cnt, eps, last);
    __syncthreads();
    // 3. award
    if (last) {                                       // the forced last step: every bidder takes its object, no eviction
      for (int k = tid; k < cnt; k += kEmdBlock) {
        const unsigned e = st.list[k];
        st.assign[e & 0xffffu] = (int)(e >> 16);
      }
    } else if constexpr (!STREAM) {
      for (int k = tid; k < cnt; k += kEmdBlock) {
        const unsigned e = st.list[k];
        const int i = (int)(e & 0xffffu), j = (int)(e >> 16);
        const unsigned long long key = st.key[j];
        if ((unsigned)key == 0xffffffffu - (unsigned)i) {
          const int old = st.owner[j];
          if (old >= 0) st.assign[old] = -1;
          st.owner[j] = i;
          st.assign[i] = j;
          st.obj[j].w = st.obj[j].w + __uint_as_float((unsigned)(key >> 32));
        }
      }
    } else {
      for (int t0 = 0; t0 < N; t0 += kEmdTile) {
        const int tn = min(kEmdTile, N - t0);
        for (int j = tid; j < tn; j += kEmdBlock) st.key[j] = 0ull;
        __syncthreads();
        for (int k = tid; k < cnt; k += kEmdBlock) {
          const unsigned e = st.list[k];
          const int j = (int)(e >> 16) - t0;
          if (j >= 0 && j < tn) atomicMax(&st.key[j], emd_key(st.inc[k], (int)(e & 0xffffu)));
        }
        __syncthreads();
        for (int k = tid; k < cnt; k += kEmdBlock) {
          const unsigned e = st.list[k];
          const int i = (int)(e & 0xffffu), j = (int)(e >> 16);
          if (j < t0 || j >= t0 + tn) continue;
          const unsigned long long key = st.key[j - t0];
          if ((unsigned)key == 0xffffffffu - (unsigned)i) {
            const int old = st.owner[j];
            if (old >= 0) st.assign[old] = -1;
            st.owner[j] = i;
            st.assign[i] = j;
            st.price[j] = st.price[j] + __uint_as_float((unsigned)(key >> 32));
          }
        }
        __syncthreads();
      }
    }
    __syncthreads();
  }
  if (tid == 0 && iters_run) iters_run[b] = t;
  // 4. output: squared distance to the assigned object (reference CalcDist)
  for (int i = tid; i < N; i += kEmdBlock) {
    const int j = st.assign[i];
    const float dx = p1[i * 3 + 0] - p2[j * 3 + 0], dy = p1[i * 3 + 1] - p2[j * 3 + 1], dz = p1[i * 3 + 2] - p2[j * 3 + 2];
    dist[(size_t)b * N + i] = (dx * dx + dy * dy) + dz * dz;
    assignment[(size_t)b * N + i] = j;
  }
}

__global__ __launch_bounds__(256) void emd_backward_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                           size_t total, int N, const float* __restrict__ graddist,
                                                           const int* __restrict__ assignment, float* __restrict__ gradxyz1) {
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t b = e / N;
    const size_t j = b * N + (size_t)assignment[e];
    const float g = graddist[e] * 2.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) gradxyz1[e * 3 + c] += g * (xyz1[e * 3 + c] - xyz2[j * 3 + c]);
  }
}

size_t emd_lds_bytes(int N) {
  const size_t tile = N <= kEmdTile ? (size_t)emd_stride(N) : (size_t)kEmdTile;
  return 24 * tile + 16 + (N <= kEmdTile ? 12 * (size_t)emd_stride(N) : 0);
}

}  // namespace
}  // namespace houv

extern "C" long long houv_emd_workspace_bytes(int B, int N) {
  using namespace houv;
  if (B <= 0 || N <= kEmdTile || N > kEmdMaxN) return 0;
  return (long long)B * 20 * emd_stride(N);
}

extern "C" int houv_emd_forward(const float* xyz1, const float* xyz2, int B, int N, int M, float eps, int iters, float* dist,
                                int32_t* assignment, int32_t* iters_run_or_null, void* workspace_or_null, void* stream) {
  using namespace houv;
  if (B < 0 || N < 1 || N > kEmdMaxN || N != M || iters < 1 || !(eps > 0.f) || !(eps < INFINITY)) {
    set_error("houv_emd_forward: bad argument B=%d N=%d M=%d eps=%g iters=%d (need N == M in 1..%d, eps > 0, iters >= 1)", B,
              N, M, (double)eps, iters, kEmdMaxN);
    return 0;
  }
  if (B == 0) return 1;
  if (!xyz1 || !xyz2 || !dist || !assignment) { set_error("houv_emd_forward: null pointer"); return 0; }
  const bool stream_kernel = N > kEmdTile;
  if (stream_kernel && !workspace_or_null) {
    set_error("houv_emd_forward: N=%d > %d needs a workspace of houv_emd_workspace_bytes(B, N) bytes", N, kEmdTile);
    return 0;
  }
  const size_t lds = emd_lds_bytes(N);
  const void* fn = stream_kernel ? (const void*)emd_auction_kernel<true> : (const void*)emd_auction_kernel<false>;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    set_error("houv_emd_forward: %zu B of LDS: %s", lds, hipGetErrorString(e));
    return 0;
  }
  hipStream_t s = (hipStream_t)stream;
  if (stream_kernel)
    emd_auction_kernel<true><<<B, kEmdBlock, lds, s>>>(xyz1, xyz2, N, eps, iters, dist, assignment, iters_run_or_null,
                                                       (unsigned char*)workspace_or_null);
  else
    emd_auction_kernel<false><<<B, kEmdBlock, lds, s>>>(xyz1, xyz2, N, eps, iters, dist, assignment, iters_run_or_null,
                                                        nullptr);
  return check_launch("houv_emd_forward") ? 1 : 0;
}

extern "C" int houv_emd_backward(const float* xyz1, const float* xyz2, int B, int N, const float* graddist,
                                 const int32_t* assignment, float* gradxyz1, void* stream) {
  using namespace houv;
  if (B < 0 || N < 1 || N > kEmdMaxN) {
    set_error("houv_emd_backward: bad argument B=%d N=%d", B, N);
    return 0;
  }
  if (B == 0) return 1;
  if (!xyz1 || !xyz2 || !graddist || !assignment || !gradxyz1) { set_error("houv_emd_backward: null pointer"); return 0; }
  const size_t total = (size_t)B * N;
  size_t blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  emd_backward_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(xyz1, xyz2, total, N, graddist, assignment, gradxyz1);
  return check_launch("houv_emd_backward") ? 1 : 0;
}
