// kd_sort.hip -- houv_kd_sort: the k-d leaf order of houv_amd.solver.kd_sort, one workgroup per cloud, all in LDS.
//
// The point order the pruned search wants (houv_solve_iterate_pruned): consecutive runs of `leaf` points are the leaves of a
// balanced k-d tree.  Bit for bit the permutation solver.kd_sort computes with torch on the same device:
//   - start: lexicographic (x, y, z), ties in input order = three stable sorts by z, y, x;
//   - level by level, every segment of more than one tile (tiles = ceil(len / leaf)) is cut at a + (tiles - tiles/2) * leaf and
//     reordered, stably, along one axis: rule 0 ("area") the axis whose two halves have the smallest summed projected box areas
//     (axis 0 first, a later one only if strictly smaller), rule 1 ("extent") the first axis of the largest max - min.
// Points never move in LDS; a permutation (input index per position) does.  Every stable sort is ONE bitonic sort of 64-bit keys
// (segment start | orderable coordinate | current position) over the padded power-of-two array: the position field makes the
// network stable and the segment field keeps all segments of a level, ragged ones included, in place.  Segments that are not cut
// get coordinate field 0 and keep their order.
//
// torch's stable sort of <= 4096 keys on this device is a block radix sort on the raw float bits (rocPRIM's key codec): -0 and
// +0 compare equal, a NaN sorts by its bits -- positive NaNs above +Inf, negative ones below -Inf.  ord_key reproduces exactly
// that.  Box extents use NaN-propagating max / min (torch's max / min along a dimension) and the area sums are evaluated in
// torch's order without contraction (-ffp-contract=off), so a NaN cost never wins a `<`, as in torch.where(cost < best, ...).
#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kKdMax = 4096;               // points per cloud (12-bit position and segment fields)
constexpr int kKdNodes = kKdMax / 2;       // nodes of one tree level that can be cut (each has >= 2 tiles)
constexpr int kKdBlock = 1024;

// rocPRIM's radix key of a float, -0 folded onto +0: an unsigned order equal to the float order for non-NaN values
__device__ __forceinline__ uint32_t ord_key(float f) {
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// torch's max / min reductions: a NaN anywhere gives NaN (fmaxf / fminf would drop it)
__device__ __forceinline__ float nan_max(float a, float b) { return (a != a || a > b) ? a : b; }
__device__ __forceinline__ float nan_min(float a, float b) { return (a != a || a < b) ? a : b; }

// A node of tree level L: tiles [ta, tb), path index j among the 2^L slots of that level, cut tile tm (split only)
struct KdNode {
  int ta, tb, tm, j;
  bool split;
};

// The node of level L holding tile t, or the leaf above level L that holds it (split = false)
__device__ __forceinline__ KdNode node_of_tile(int t, int L, int T) {
  KdNode n{0, T, 0, 0, false};
  for (int d = 0; d <= L; ++d) {
    const int tiles = n.tb - n.ta;
    if (tiles <= 1) return n;
    const int tm = n.ta + (tiles - tiles / 2);      // the left half gets the extra tile
    if (d == L) {
      n.tm = tm;
      n.split = true;
      return n;
    }
    if (t < tm) { n.tb = tm; n.j = 2 * n.j; }
    else        { n.ta = tm; n.j = 2 * n.j + 1; }
  }
  return n;
}

// Slot j of level L, descended along the bits of j; split = false when no node of level L sits there or it is a leaf
__device__ __forceinline__ KdNode node_of_slot(int j, int L, int T) {
  KdNode n{0, T, 0, j, false};
  for (int d = 0; d <= L; ++d) {
    const int tiles = n.tb - n.ta;
    if (tiles <= 1) return n;
    const int tm = n.ta + (tiles - tiles / 2);
    if (d == L) {
      n.tm = tm;
      n.split = true;
      return n;
    }
    if ((j >> (L - 1 - d)) & 1) n.ta = tm;
    else n.tb = tm;
  }
  return n;
}

// One compare-exchange stage (merge size k, distance j) over the first `pad` keys in LDS, then a barrier
__device__ __forceinline__ void lds_stage(uint64_t* key, int pad, int k, int j) {
  for (int t = threadIdx.x; t < pad / 2; t += kKdBlock) {
    const int i = 2 * t - (t & (j - 1));
    const uint64_t a = key[i], b = key[i + j];
    if ((a > b) == ((i & k) == 0)) {
      key[i] = b;
      key[i + j] = a;
    }
  }
  __syncthreads();
}

// Stage (k, j < 64) on a key held by lane e % 64: the partner e ^ j sits in the same register of lane ^ j
__device__ __forceinline__ uint64_t lane_stage(uint64_t v, int e, int k, int j) {
  const uint32_t lo = __shfl_xor((uint32_t)v, j, kWave), hi = __shfl_xor((uint32_t)(v >> 32), j, kWave);
  const uint64_t w = ((uint64_t)hi << 32) | lo;
  const bool keep_min = ((e & j) == 0) == ((e & k) == 0);
  return keep_min ? (v < w ? v : w) : (v < w ? w : v);
}

// Stages j = j_top .. 1 of merge size k (kk = k, or every k from 2 to 128 when k == 0) for every 128-key chunk, in registers:
// lane l of the wave holds keys c + l and c + 64 + l.  No barrier between stages.
__device__ __forceinline__ void chunk_stages(uint64_t* key, int pad, int k, int j_top) {
  const int lane = threadIdx.x % kWave;
  for (int c = (threadIdx.x / kWave) * 128; c < pad; c += kKdBlock * 2) {
    const int e0 = c + lane, e1 = e0 + 64;
    uint64_t v0 = key[e0], v1 = key[e1];
    for (int kk = k ? k : 2; kk <= (k ? k : 128); kk <<= 1) {
      for (int j = k ? j_top : kk >> 1; j > 0; j >>= 1) {
        if (j == 64) {
          if ((v0 > v1) == ((e0 & kk) == 0)) { const uint64_t t = v0; v0 = v1; v1 = t; }
        } else {
          v0 = lane_stage(v0, e0, kk, j);
          v1 = lane_stage(v1, e1, kk, j);
        }
      }
    }
    key[e0] = v0;
    key[e1] = v1;
  }
  __syncthreads();
}

// Stable sort of the first `pad` (a power of two) keys, ascending; every thread of the block takes part.  Distances of 128 and
// more go through LDS with a barrier per stage; the shorter ones of each merge run in registers, within a wave.  Not inlined:
// inlined at its three call sites it made the kernel spill SGPRs.
__device__ __attribute__((noinline)) void bitonic_sort(uint64_t* key, int pad) {
  if (pad < 128) {
    for (int k = 2; k <= pad; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) lds_stage(key, pad, k, j);
    return;
  }
  chunk_stages(key, pad, 0, 0);
  for (int k = 256; k <= pad; k <<= 1) {
    for (int j = k >> 1; j >= 128; j >>= 1) lds_stage(key, pad, k, j);
    chunk_stages(key, pad, k, 64);
  }
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_max(v, __shfl_xor(v, o, kWave));
  return v;
}
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = nan_min(v, __shfl_xor(v, o, kWave));
  return v;
}

__global__ __launch_bounds__(kKdBlock) void kd_sort_kernel(const float* __restrict__ xyz, int N, int leaf, int rule,
                                                             float* __restrict__ out, int32_t* __restrict__ order) {
  __shared__ float pts[3][kKdMax];           // the cloud, by input index
  __shared__ uint64_t key[kKdMax];           // sort keys: (segment start << 44) | (ord_key << 12) | position
  __shared__ uint16_t perm_buf[2][kKdMax];   // input index of the point at each position: current / next
  __shared__ float best[kKdNodes];           // area rule: smallest cost so far per node of the level
  __shared__ uint8_t pick[kKdNodes];         // area rule: the last candidate won; extent rule: the split axis

  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  constexpr int kWaves = kKdBlock / kWave;
  const size_t cloud = blockIdx.x;
  const float* in = xyz + cloud * N * 3;
  for (int e = tid; e < 3 * N; e += kKdBlock) pts[e % 3][e / 3] = in[e];
  for (int i = tid; i < N; i += kKdBlock) perm_buf[0][i] = (uint16_t)i;
  int pad = 1;
  while (pad < N) pad <<= 1;
  uint16_t* perm = perm_buf[0];
  uint16_t* next = perm_buf[1];
  __syncthreads();

  // lexicographic (x, y, z): stable sorts by z, then y, then x
  for (int ax = 2; ax >= 0; --ax) {
    for (int i = tid; i < pad; i += kKdBlock)
      key[i] = i < N ? ((uint64_t)ord_key(pts[ax][perm[i]]) << 12) | (uint64_t)i : ~0ull;
    __syncthreads();
    bitonic_sort(key, pad);
    for (int i = tid; i < N; i += kKdBlock) next[i] = perm[key[i] & 0xFFF];
    __syncthreads();
    uint16_t* t = perm; perm = next; next = t;
  }

  const int T = (N - 1) / leaf + 1;          // tiles; the host caps leaf at N, so T * leaf < 2 N
  // keys of one candidate sort of level L: cut nodes along `ax` (extent rule: their own axis in pick[]), the rest in place
  auto build_keys = [&](int L, int ax) {
    for (int i = tid; i < pad; i += kKdBlock) {
      uint64_t k = ~0ull;
      if (i < N) {
        const KdNode n = node_of_tile(i / leaf, L, T);
        const int a = n.ta * leaf;
        const int axis = rule == 0 ? ax : pick[n.j];
        const uint32_t c = n.split ? ord_key(pts[axis][perm[i]]) : 0u;
        k = ((uint64_t)a << 44) | ((uint64_t)c << 12) | (uint64_t)i;
      }
      key[i] = k;
    }
    __syncthreads();
  };

  for (int L = 0, widest = T; widest > 1; ++L, widest -= widest / 2) {
    const int slots = 1 << L;
    if (rule == 0) {
      for (int ax = 0; ax < 3; ++ax) {
        build_keys(L, ax);
        bitonic_sort(key, pad);
        // cost of this candidate per cut node: one wave per node, boxes of both halves in the candidate order
        for (int j = wave; j < slots; j += kWaves) {
          const KdNode n = node_of_slot(j, L, T);
          if (!n.split) continue;
          const int a = n.ta * leaf, m = n.tm * leaf, b = min(n.tb * leaf, N);
          float lo[2][3], hi[2][3];
#pragma unroll
          for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < 3; ++c) { lo[h][c] = __builtin_inff(); hi[h][c] = -__builtin_inff(); }
          for (int i = a + lane; i < b; i += kWave) {
            const int p = perm[key[i] & 0xFFF];
            const bool right = i >= m;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const float v = pts[c][p];
              if (right) { lo[1][c] = nan_min(lo[1][c], v); hi[1][c] = nan_max(hi[1][c], v); }
              else       { lo[0][c] = nan_min(lo[0][c], v); hi[0][c] = nan_max(hi[0][c], v); }
            }
          }
          float area[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            float e[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) e[c] = wave_max(hi[h][c]) - wave_min(lo[h][c]);
            area[h] = (e[0] * e[1] + e[1] * e[2]) + e[0] * e[2];      // solver._split_segments' order; no contraction
          }
          const float cost = area[0] + area[1];
          if (lane == 0) {
            const bool take = ax == 0 || cost < best[j];
            if (take) best[j] = cost;
            pick[j] = take;
          }
        }
        __syncthreads();
        for (int i = tid; i < N; i += kKdBlock) {
          const KdNode n = node_of_tile(i / leaf, L, T);
          if (ax == 0 || (n.split && pick[n.j])) next[i] = perm[key[i] & 0xFFF];
        }
        __syncthreads();
      }
    } else {
      // split axis per cut node: argmax of max - min, a NaN extent first, else the first largest
      for (int j = wave; j < slots; j += kWaves) {
        const KdNode n = node_of_slot(j, L, T);
        if (!n.split) continue;
        const int a = n.ta * leaf, b = min(n.tb * leaf, N);
        float lo[3], hi[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { lo[c] = __builtin_inff(); hi[c] = -__builtin_inff(); }
        for (int i = a + lane; i < b; i += kWave) {
          const int p = perm[i];
#pragma unroll
          for (int c = 0; c < 3; ++c) { lo[c] = nan_min(lo[c], pts[c][p]); hi[c] = nan_max(hi[c], pts[c][p]); }
        }
        int axis = 0;
        float top = wave_max(hi[0]) - wave_min(lo[0]);
#pragma unroll
        for (int c = 1; c < 3; ++c) {
          const float e = wave_max(hi[c]) - wave_min(lo[c]);
          if (top == top && (e != e || e > top)) { top = e; axis = c; }
        }
        if (lane == 0) pick[j] = (uint8_t)axis;
      }
      __syncthreads();
      build_keys(L, 0);
      bitonic_sort(key, pad);
      for (int i = tid; i < N; i += kKdBlock) next[i] = perm[key[i] & 0xFFF];
      __syncthreads();
    }
    uint16_t* t = perm; perm = next; next = t;
  }

  float* o = out + cloud * N * 3;
  for (int e = tid; e < 3 * N; e += kKdBlock) o[e] = pts[e % 3][perm[e / 3]];
  if (order)
    for (int i = tid; i < N; i += kKdBlock) order[cloud * N + i] = perm[i];
}

}  // namespace
}  // namespace houv

extern "C" int houv_kd_sort(const float* xyz, int P, int N, int leaf, int rule, float* out, int32_t* order, void* stream) {
  using namespace houv;
  if (P < 0 || N < 1 || N > kKdMax) {
    set_error("houv_kd_sort: bad shape P=%d N=%d (1 <= N <= %d)", P, N, kKdMax);
    return 0;
  }
  if (leaf < 1) {
    set_error("houv_kd_sort: leaf must be >= 1 (got %d)", leaf);
    return 0;
  }
  if (rule != 0 && rule != 1) {
    set_error("houv_kd_sort: unknown rule %d (0 = area, 1 = extent)", rule);
    return 0;
  }
  if (P == 0) return 1;
  if (!xyz || !out) {
    set_error("houv_kd_sort: null pointer");
    return 0;
  }
  // a cloud is read from xyz while the sorted one is written to out (and order): none may overlap another
  const uintptr_t x0 = (uintptr_t)xyz, o0 = (uintptr_t)out, r0 = (uintptr_t)order;
  const uintptr_t bytes = (uintptr_t)P * N * 3 * sizeof(float), obytes = (uintptr_t)P * N * sizeof(int32_t);
  auto overlap = [](uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a == b || (a < b + nb && b < a + na); };
  if (overlap(x0, bytes, o0, bytes)) {
    set_error("houv_kd_sort: out overlaps xyz (the sort is not in place)");
    return 0;
  }
  if (order && (overlap(r0, obytes, x0, bytes) || overlap(r0, obytes, o0, bytes))) {
    set_error("houv_kd_sort: order overlaps xyz or out");
    return 0;
  }
  kd_sort_kernel<<<P, kKdBlock, 0, (hipStream_t)stream>>>(xyz, N, leaf < N ? leaf : N, rule, out, order);
  return check_launch("houv_kd_sort") ? 1 : 0;
}
