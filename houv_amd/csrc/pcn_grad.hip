// pcn_grad.hip -- houv_mlp2_max_backward: the backward pass of one PointNet block (houv_mlp2_max_arg).
//
// The maximum over the points sends the gradient of pooled[b,c] to the single row arg[b,c], so everything is evaluated on the
// ACTIVE rows A_b = set(arg[b,:]) u rows[b] only, compacted per cloud into Rcap = min(N, Cout + R) slots (ascending rows, zero
// padding): the hidden activations are recomputed there, the one-hot part of gz is never built (its share of gW2 and gh is one
// axpy per pooled channel), and the two real products (gW1, gx) and the recomputation go through houv_gemm_f32.  Every sum has
// a fixed order and nothing is atomic: two calls give the same bits.
#include <algorithm>
#include <cstdio>

#include "../../include/houv_hip.h"
#include "houv_common.h"

namespace houv {
namespace {

constexpr int kBT = 256;                         // threads of the bookkeeping kernels

struct BwShape {
  int B, N, Cin, H, Cout, R, Rcap, S, cps;       // S chunks of cps clouds for the gW2 partials
  int KC, SK;                                    // the gW1 product: SK chunks of KC slots each, whatever B is
  long long slots, slotsP;                       // B * Rcap, and that rounded up to SK * KC (the slots past B * Rcap are empty)
};

// position in the ascending list rows[0 .. n) of value r, or -1
__device__ __forceinline__ int find_row(const int* __restrict__ rows, int n, int r) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (rows[mid] < r) lo = mid + 1; else hi = mid;
  }
  return (lo < n && rows[lo] == r) ? lo : -1;
}

// One workgroup per cloud: pos[b,n] = slot of row n among the active rows of cloud b (-1: not active), act_rows[b,slot] = n
// ascending (-1 past the last), nact[b], lpos[b,k] = slot of the listed row rows[b,k].
__global__ __launch_bounds__(kBT) void pcn_bw_rows_kernel(const int* __restrict__ arg, const int* __restrict__ rows,
                                                          const int* __restrict__ nrows, int* __restrict__ pos,
                                                          int* __restrict__ lpos, int* __restrict__ act_rows,
                                                          int* __restrict__ nact, const BwShape s) {
  __shared__ int scan[kBT];
  const int b = blockIdx.x, tid = threadIdx.x;
  int* pb = pos + (size_t)b * s.N;
  for (int n = tid; n < s.N; n += kBT) pb[n] = 0;
  __syncthreads();
  for (int c = tid; c < s.Cout; c += kBT) {
    const int a = arg[(size_t)b * s.Cout + c];
    if ((unsigned)a < (unsigned)s.N) pb[a] = 1;  // -1 (an all-NaN column) and anything out of range: no row
  }
  const int nr = rows ? min(max(nrows[b], 0), s.R) : 0;
  for (int k = tid; k < nr; k += kBT) {
    const int r = rows[(size_t)b * s.R + k];
    if ((unsigned)r < (unsigned)s.N) pb[r] = 1;
  }
  __syncthreads();
  int running = 0;
  for (int n0 = 0; n0 < s.N; n0 += kBT) {
    const int n = n0 + tid;
    const int f = n < s.N ? pb[n] : 0;
    scan[tid] = f;
    __syncthreads();
    for (int o = 1; o < kBT; o <<= 1) {
      const int v = tid >= o ? scan[tid - o] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const int p = running + scan[tid] - f;
    if (n < s.N) pb[n] = f ? p : -1;
    if (f && p < s.Rcap) act_rows[(size_t)b * s.Rcap + p] = n;
    running += scan[kBT - 1];
    __syncthreads();
  }
  for (int p = running + tid; p < s.Rcap; p += kBT) act_rows[(size_t)b * s.Rcap + p] = -1;
  if (tid == 0) nact[b] = min(running, s.Rcap);
  for (int k = tid; k < s.R; k += kBT) {
    int v = -1;
    if (k < nr) {
      const int r = rows[(size_t)b * s.R + k];
      if ((unsigned)r < (unsigned)s.N) v = pb[r];
    }
    lpos[(size_t)b * s.R + k] = v;
  }
}

// xa[b,p,:] = x[b, act_rows[b,p], :], zeros in the padding slots
__global__ __launch_bounds__(kBT) void pcn_bw_gather_kernel(const float* __restrict__ x, const int* __restrict__ act_rows,
                                                            float* __restrict__ xa, long long total, const BwShape s) {
  const long long o = (long long)blockIdx.x * kBT + threadIdx.x;
  if (o >= total) return;
  const long long slot = o / s.Cin;              // b * Rcap + p
  const int k = (int)(o - slot * s.Cin);
  const long long b = slot / s.Rcap;
  const int r = slot < s.slots ? act_rows[slot] : -1;
  xa[o] = r >= 0 ? x[((size_t)b * s.N + r) * s.Cin + k] : 0.f;
}

// One workgroup per slot (b, p), the empty ones past B * Rcap included (they store zeros): gh[b,p,:] = (sum over c ascending of gz[b,r,c] W2[c,:]) * [h[b,p,:] > 0] with
// gz[b,r,c] = gy[b,r,c] + gpooled[b,c] [arg[b,c] == r], also stored k-major (ghT[ch, b*Rcap + p]).  Terms with gz == 0 are
// skipped: a row that only the maximum reaches costs one axpy per pooled channel that points at it.
template <int CPT>                               // hidden channels per thread: H = 128 * CPT
__global__ __launch_bounds__(128) void pcn_bw_gh_kernel(const float* __restrict__ W2, const int* __restrict__ arg,
                                                        const float* __restrict__ gpooled, const int* __restrict__ rows,
                                                        const int* __restrict__ nrows, const float* __restrict__ gy_rows,
                                                        const int* __restrict__ act_rows, const float* __restrict__ h,
                                                        float* __restrict__ gh, float* __restrict__ ghT, const BwShape s) {
  const long long slot = blockIdx.x;
  const int b = (int)(slot / s.Rcap), tid = threadIdx.x;
  const int r = slot < s.slots ? act_rows[slot] : -1;
  const long long ld = s.slotsP;
  float acc[CPT];
#pragma unroll
  for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
  if (r >= 0) {
    const int nr = rows ? min(max(nrows[b], 0), s.R) : 0;
    const int k = nr ? find_row(rows + (size_t)b * s.R, nr, r) : -1;
    const float* gyr = k >= 0 ? gy_rows + ((size_t)b * s.R + k) * s.Cout : nullptr;
    const int* ab = arg + (size_t)b * s.Cout;
    const float* gpb = gpooled + (size_t)b * s.Cout;
    for (int c = 0; c < s.Cout; ++c) {
      float gz = gyr ? gyr[c] : 0.f;
      if (ab[c] == r) gz += gpb[c];
      if (gz != 0.f) {
#pragma unroll
        for (int i = 0; i < CPT; ++i) acc[i] = __builtin_fmaf(gz, W2[(size_t)c * s.H + tid + 128 * i], acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i) {
    const int ch = tid + 128 * i;
    const float g = (r >= 0 && h[slot * s.H + ch] > 0.f) ? acc[i] : 0.f;
    gh[slot * s.H + ch] = g;
    ghT[ch * ld + slot] = g;
  }
}

// Workgroup (c, chunk): the chunk's share of gW2[c,:] = sum over b, r of gz[b,r,c] h[b,r,:] and of gb2[c] = sum of gz[b,r,c],
// clouds ascending and, inside a cloud, the arg-max row first when it is not a listed one, then the listed rows ascending.
template <int CPT>
__global__ __launch_bounds__(128) void pcn_bw_gw2_kernel(const int* __restrict__ arg, const float* __restrict__ gpooled,
                                                         const int* __restrict__ rows, const int* __restrict__ nrows,
                                                         const float* __restrict__ gy_rows, const int* __restrict__ pos,
                                                         const int* __restrict__ lpos, const float* __restrict__ h,
                                                         float* __restrict__ gW2p, float* __restrict__ gb2p, const BwShape s) {
  const int c = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x;
  float acc[CPT], gb = 0.f;
#pragma unroll
  for (int i = 0; i < CPT; ++i) acc[i] = 0.f;
  const int b1 = min(s.B, (chunk + 1) * s.cps);
  for (int b = chunk * s.cps; b < b1; ++b) {
    const int a = arg[(size_t)b * s.Cout + c];
    const float gp = gpooled[(size_t)b * s.Cout + c];
    const bool live = (unsigned)a < (unsigned)s.N;
    const int nr = rows ? min(max(nrows[b], 0), s.R) : 0;
    const int ka = (live && nr) ? find_row(rows + (size_t)b * s.R, nr, a) : -1;
    if (live && ka < 0) {
      const float* hr = h + ((size_t)b * s.Rcap + pos[(size_t)b * s.N + a]) * s.H;
      gb += gp;
#pragma unroll
      for (int i = 0; i < CPT; ++i) acc[i] = __builtin_fmaf(gp, hr[tid + 128 * i], acc[i]);
    }
#pragma unroll 4
    for (int k = 0; k < nr; ++k) {
      const int p = lpos[(size_t)b * s.R + k];
      float gz = gy_rows[((size_t)b * s.R + k) * s.Cout + c];
      if (k == ka) gz += gp;
      if (p >= 0) {
        const float* hr = h + ((size_t)b * s.Rcap + p) * s.H;
        gb += gz;
#pragma unroll
        for (int i = 0; i < CPT; ++i) acc[i] = __builtin_fmaf(gz, hr[tid + 128 * i], acc[i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < CPT; ++i) gW2p[((size_t)chunk * s.Cout + c) * s.H + tid + 128 * i] = acc[i];
  if (tid == 0) gb2p[(size_t)chunk * s.Cout + c] = gb;
}

// out[i] = sum over s < S of part[s * n + i], s ascending
__global__ __launch_bounds__(kBT) void pcn_bw_fold_kernel(const float* __restrict__ part, int S, long long n,
                                                          float* __restrict__ out) {
  const long long i = (long long)blockIdx.x * kBT + threadIdx.x;
  if (i >= n) return;
  float v = part[i];
  for (int k = 1; k < S; ++k) v += part[(size_t)k * n + i];
  out[i] = v;
}

// gshift1[b, ch] = sum over the slots p < nact[b] of gh[b,p,ch], p ascending
__global__ __launch_bounds__(kBT) void pcn_bw_gshift_kernel(const float* __restrict__ gh, const int* __restrict__ nact,
                                                            float* __restrict__ gshift1, long long total, const BwShape s) {
  const long long o = (long long)blockIdx.x * kBT + threadIdx.x;
  if (o >= total) return;
  const long long b = o / s.H;
  const int ch = (int)(o - b * s.H);
  const float* g = gh + (size_t)b * s.Rcap * s.H + ch;
  const int n = nact[b];
  float v = 0.f;
  for (int p = 0; p < n; ++p) v += g[(size_t)p * s.H];
  gshift1[o] = v;
}

inline long long up4(long long n) { return (n + 3) & ~3LL; }

struct BwLayout {                                // offsets into the workspace, in 4-byte elements, each a multiple of 4
  long long pos, lpos, xa, h, gh, ghT, gW2p, gb2p, gW1p, total;
};

BwLayout layout(const BwShape& s) {
  BwLayout l;
  long long o = 0;
  const long long slots = s.slotsP;
  l.pos = o; o += up4((long long)s.B * s.N);
  l.lpos = o; o += up4((long long)s.B * s.R);
  l.xa = o; o += up4(slots * s.Cin);
  l.h = o; o += up4(slots * s.H);
  l.gh = o; o += up4(slots * s.H);
  l.ghT = o; o += up4(slots * s.H);
  l.gW2p = o; o += up4((long long)s.S * s.Cout * s.H);
  l.gb2p = o; o += up4((long long)s.S * s.Cout);
  l.gW1p = o; o += up4((long long)s.SK * s.H * s.Cin);
  l.total = o;
  return l;
}

BwShape shape(int B, int N, int Cin, int H, int Cout, int R) {
  BwShape s{B, N, Cin, H, Cout, R, 0, 1, 1};
  s.Rcap = (int)std::min<long long>(N, (long long)Cout + R);
  const long long per = (long long)Cout * H;     // at most 4 Mi floats of gW2 partials
  s.S = (int)std::max<long long>(1, std::min<long long>(B, (4LL << 20) / per));
  s.cps = (B + s.S - 1) / std::max(s.S, 1);
  s.S = s.cps ? (B + s.cps - 1) / s.cps : 1;
  // gW1 has a small output and a long reduction over the slots: split the slots into about 32 chunks (a multiple of 32 slots
  // each, so that full tiles stay 16-byte aligned), which with the 4 x 2 .. 4 x 4 output tiles fills the device at any B
  s.slots = (long long)B * s.Rcap;
  s.KC = (int)std::max<long long>(32, ((s.slots + 31) / 32 + 31) / 32 * 32);
  s.SK = (int)((s.slots + s.KC - 1) / s.KC);
  s.slotsP = (long long)s.SK * s.KC;
  return s;
}

const char* check_shape(int B, int N, int Cin, int H, int Cout, int R) {
  static thread_local char msg[256];
  if (B < 0 || N < 1 || R < 0) {
    snprintf(msg, sizeof msg, "bad shape B=%d N=%d R=%d (N >= 1, R >= 0)", B, N, R);
    return msg;
  }
  const bool first = Cin == 3 && H == 128 && Cout == 256, second = Cin == 256 && H == 512 && Cout == 1024;
  if (!first && !second) {
    snprintf(msg, sizeof msg, "(Cin, H, Cout) = (%d, %d, %d) has no kernel: (3, 128, 256) and (256, 512, 1024) are served", Cin, H,
             Cout);
    return msg;
  }
  const long long rcap = std::min<long long>(N, (long long)Cout + R);
  if (B > 65535 || (long long)B * rcap > 128LL * 65535 - 4096 || (long long)B * rcap * H > 0x7fffffffLL || (long long)B * N > 0x7fffffffLL) {
    snprintf(msg, sizeof msg, "B=%d x N=%d is too large for one call (B <= 65535, B * min(N, Cout + R) <= 8384384)", B, N);
    return msg;
  }
  return nullptr;
}

}  // namespace
}  // namespace houv

extern "C" int houv_mlp2_max_backward_rows(int N, int Cout, int R) {
  if (N < 1 || Cout < 1 || R < 0) return 0;
  return (int)std::min<long long>(N, (long long)Cout + R);
}

extern "C" long long houv_mlp2_max_backward_workspace_bytes(int B, int N, int Cin, int H, int Cout, int R) {
  using namespace houv;
  if (B <= 0 || check_shape(B, N, Cin, H, Cout, R)) return 0;
  return layout(shape(B, N, Cin, H, Cout, R)).total * 4;
}

extern "C" int houv_mlp2_max_backward(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
                                      long long shift1_stride, const float* W2, int Cout, const int32_t* arg,
                                      const float* gpooled, const int32_t* rows_or_null, const int32_t* nrows_or_null,
                                      const float* gy_rows_or_null, int R, float* gW1, float* gshift1, float* gW2, float* gb2,
                                      int32_t* act_rows, int32_t* nact, float* gx_rows_or_null, void* workspace, void* stream) {
  using namespace houv;
  if (const char* why = check_shape(B, N, Cin, H, Cout, R)) {
    set_error("houv_mlp2_max_backward: %s", why);
    return 0;
  }
  if (shift1_stride != 0 && shift1_stride < H) {
    set_error("houv_mlp2_max_backward: shift1_stride=%lld must be 0 (one shared row) or >= H=%d", shift1_stride, H);
    return 0;
  }
  {
    const void* req[] = {x, W1, shift1, W2, arg, gpooled, gW1, gshift1, gW2, gb2, act_rows, nact, workspace};
    const char* names[] = {"x", "W1", "shift1", "W2", "arg", "gpooled", "gW1", "gshift1", "gW2", "gb2", "act_rows", "nact", "workspace"};
    for (int i = 0; i < 13; ++i)
      if (!req[i]) {
        set_error("houv_mlp2_max_backward: %s is a null pointer", names[i]);
        return 0;
      }
    if (R > 0 && (!rows_or_null || !nrows_or_null || !gy_rows_or_null)) {
      set_error("houv_mlp2_max_backward: R=%d but rows, nrows or gy_rows is a null pointer", R);
      return 0;
    }
  }
  hipStream_t st = (hipStream_t)stream;
  const long long wsize = (long long)H * Cin, w2size = (long long)Cout * H;
  if (B == 0) {                                  // no cloud: the weight gradients are zero
    if (hipMemsetAsync(gW1, 0, wsize * 4, st) != hipSuccess || hipMemsetAsync(gW2, 0, w2size * 4, st) != hipSuccess ||
        hipMemsetAsync(gb2, 0, (size_t)Cout * 4, st) != hipSuccess) {
      set_error("houv_mlp2_max_backward: hipMemsetAsync failed");
      return 0;
    }
    return 1;
  }
  const BwShape s = shape(B, N, Cin, H, Cout, R);
  const BwLayout l = layout(s);
  const int32_t* rows = R > 0 ? rows_or_null : nullptr;
  float* wf = static_cast<float*>(workspace);
  int* wi = static_cast<int*>(workspace);
  int *pos = wi + l.pos, *lpos = wi + l.lpos;
  float *xa = wf + l.xa, *h = wf + l.h, *gh = wf + l.gh, *ghT = wf + l.ghT, *gW2p = wf + l.gW2p, *gb2p = wf + l.gb2p, *gW1p = wf + l.gW1p;
  const long long slots = s.slots;
  auto blocks = [](long long n) { return (unsigned)((n + kBT - 1) / kBT); };
  const char* fn = "houv_mlp2_max_backward";

  pcn_bw_rows_kernel<<<(unsigned)B, kBT, 0, st>>>(arg, rows, nrows_or_null, pos, lpos, act_rows, nact, s);
  if (!check_launch(fn)) return 0;
  pcn_bw_gather_kernel<<<blocks(s.slotsP * Cin), kBT, 0, st>>>(x, act_rows, xa, s.slotsP * Cin, s);
  if (!check_launch(fn)) return 0;
  // h = relu(xa W1^T + shift1[b]) per cloud: the per-cloud shift enters as a residual of row stride 0
  if (!houv_gemm_f32(xa, W1, h, s.Rcap, H, Cin, Cin, Cin, H, 1, B, 1, (long long)s.Rcap * Cin, 0, 0, 0, (long long)s.Rcap * H, 0, 1.f,
                     nullptr, nullptr, shift1, 0, shift1_stride, 0, 1, stream))
    return 0;
  if (H == 128) pcn_bw_gh_kernel<1><<<(unsigned)s.slotsP, 128, 0, st>>>(W2, arg, gpooled, rows, nrows_or_null, gy_rows_or_null, act_rows, h, gh, ghT, s);
  else pcn_bw_gh_kernel<4><<<(unsigned)s.slotsP, 128, 0, st>>>(W2, arg, gpooled, rows, nrows_or_null, gy_rows_or_null, act_rows, h, gh, ghT, s);
  if (!check_launch(fn)) return 0;
  {
    const dim3 grid((unsigned)Cout, (unsigned)s.S);
    if (H == 128) pcn_bw_gw2_kernel<1><<<grid, 128, 0, st>>>(arg, gpooled, rows, nrows_or_null, gy_rows_or_null, pos, lpos, h, gW2p, gb2p, s);
    else pcn_bw_gw2_kernel<4><<<grid, 128, 0, st>>>(arg, gpooled, rows, nrows_or_null, gy_rows_or_null, pos, lpos, h, gW2p, gb2p, s);
    if (!check_launch(fn)) return 0;
  }
  pcn_bw_fold_kernel<<<blocks(w2size), kBT, 0, st>>>(gW2p, s.S, w2size, gW2);
  if (!check_launch(fn)) return 0;
  pcn_bw_fold_kernel<<<blocks(Cout), kBT, 0, st>>>(gb2p, s.S, Cout, gb2);
  if (!check_launch(fn)) return 0;
  pcn_bw_gshift_kernel<<<blocks((long long)B * H), kBT, 0, st>>>(gh, nact, gshift1, (long long)B * H, s);
  if (!check_launch(fn)) return 0;
  // gW1 = gh^T xa: the slots split into SK chunks over the GEMM's outer dimension, the partials added chunks ascending
  if (!houv_gemm_f32(ghT, xa, gW1p, H, Cin, s.KC, (int)s.slotsP, Cin, Cin, 0, s.SK, 1, s.KC, 0, (long long)s.KC * Cin, 0, wsize, 0, 1.f,
                     nullptr, nullptr, nullptr, 0, 0, 0, 0, stream))
    return 0;
  pcn_bw_fold_kernel<<<blocks(wsize), kBT, 0, st>>>(gW1p, s.SK, wsize, gW1);
  if (!check_launch(fn)) return 0;
  // gx = gh W1 on the active rows
  if (gx_rows_or_null &&
      !houv_gemm_f32(gh, W1, gx_rows_or_null, (int)slots, Cin, H, H, Cin, Cin, 0, 1, 1, 0, 0, 0, 0, 0, 0, 1.f, nullptr, nullptr, nullptr,
                     0, 0, 0, 0, stream))
    return 0;
  return 1;
}
