// houv_sweep.h -- the LDS-broadcast brute-force nearest-neighbour sweep shared by the fused HOUV loop (solve.hip)
// and the ICP refinement kernel (icp.hip), plus the workgroup reduction they both use.
#pragma once
#include <type_traits>

#include "houv_common.h"

namespace houv {

typedef float houv_f4v __attribute__((ext_vector_type(4)));
typedef const houv_f4v __attribute__((address_space(3))) * lds_f4;   // LDS pointer usable from a 32-bit byte address

// Per-lane global accesses of the fused loop go through buffer resources: a uniform base (4 SGPRs) + ONE 32-bit per-lane byte
// offset shared by all of a lane's points + a uniform byte offset (the point's chunk k * BLOCK, the row of the workspace).  As
// plain pointers, LLVM hoisted one 64-bit address per point and row out of the iteration loop and spilled them to scratch
// (solve_kernel<512, 4, 4, 2>: 124 of its 192 scratch reloads, 416 B per lane).  Every access is in bounds by construction
// (callers guard with the same predicates as before); `bytes` is the size of the region.
// The thread index, opaque to the optimiser at every use: whatever the fused loop derives from it per lane (offsets, LDS
// addresses, lane masks) is recomputed where it is used, with a VALU instruction or two, instead of being hoisted out of the
// iteration loop, where it lived in a VGPR (spilled to scratch) or an SGPR pair (spilled to VGPR lanes) for the whole loop.
__device__ __forceinline__ int tid_x() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
typedef __amdgpu_buffer_rsrc_t buf_t;
__device__ __forceinline__ buf_t make_buf(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes, 0x00020000);   // raw, 32-bit data format
}

// ------------------------------------------------------------------------------------------------
// The brute-force sweep: for each of this lane's Q queries, min over all references of the NMET
// squared distances, plus the id of the 16-reference tracking unit (kTrk) that produced each minimum.
// ------------------------------------------------------------------------------------------------
// One sub-tile of the sweep: out = min(in, the sub-tile's distances), per query and metric.  `in` and `out` are DIFFERENT
// register sets (the first v_min3 of a chain is three-address: out = min3(in, a, c)), so the caller can compare out against in
// afterwards without having saved a copy.
template <int Q, int NMET>
__device__ __forceinline__ void sweep_tile(const float4* __restrict__ rp, const float (&qx)[Q], const float (&qy)[Q],
                                           const float (&qz)[Q], const float (&in)[Q][NMET], float (&out)[Q][NMET]) {
#pragma unroll
  for (int j = 0; j < kTrk; j += 2) {
    const float4 a = rp[j], c = rp[j + 1];
    // keep .w "used" so the loads stay ds_read_b128 (4 LDS cycles) instead of ds_read_b96 (8)
    asm volatile("" ::"v"(a.w), "v"(c.w));
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const float ax = a.x - qx[k], ay = a.y - qy[k], az = a.z - qz[k];
      const float cx = c.x - qx[k], cy = c.y - qy[k], cz = c.z - qz[k];
      if constexpr (NMET == 4) {
        const float axx = ax * ax, ayy = ay * ay, cxx = cx * cx, cyy = cy * cy;
        const float a3 = __builtin_fmaf(ay, ay, axx), c3 = __builtin_fmaf(cy, cy, cxx);   // z dropped
        const float a1 = __builtin_fmaf(az, az, ayy), c1 = __builtin_fmaf(cz, cz, cyy);   // x dropped
        const float a2 = __builtin_fmaf(az, az, axx), c2 = __builtin_fmaf(cz, cz, cxx);   // y dropped
        const float a0 = __builtin_fmaf(az, az, a3), c0 = __builtin_fmaf(cz, cz, c3);     // full
        out[k][0] = min3f(j == 0 ? in[k][0] : out[k][0], a0, c0);
        out[k][1] = min3f(j == 0 ? in[k][1] : out[k][1], a1, c1);
        out[k][2] = min3f(j == 0 ? in[k][2] : out[k][2], a2, c2);
        out[k][3] = min3f(j == 0 ? in[k][3] : out[k][3], a3, c3);
      } else {
        out[k][0] = min3f(j == 0 ? in[k][0] : out[k][0], metric_sqdist<0>(ax, ay, az), metric_sqdist<0>(cx, cy, cz));
      }
    }
  }
}

template <int Q, int NMET>
__device__ __forceinline__ void sweep(const float4* __restrict__ refs, int ntile, const float (&qx)[Q],
                                      const float (&qy)[Q], const float (&qz)[Q], float (&best)[Q][NMET],
                                      int (&btile)[Q][NMET]) {
  // The running minimum is threaded through the sub-tiles, ping-ponging between two register sets: per query, metric and
  // sub-tile the bookkeeping is one v_cmp + one v_cndmask ("did this sub-tile lower the minimum?"; strict <: the earlier
  // sub-tile keeps ties, so the lowest index wins) instead of v_cmp + two v_cndmask -- all half-rate instructions.
  float other[Q][NMET];
#pragma unroll
  for (int k = 0; k < Q; ++k)
#pragma unroll
    for (int m = 0; m < NMET; ++m) {
      best[k][m] = INFINITY;
      btile[k][m] = 0;
    }
  int t = 0;
  for (; t + 1 < ntile; t += 2) {
    sweep_tile<Q, NMET>(refs + t * kTrk, qx, qy, qz, best, other);
#pragma unroll
    for (int k = 0; k < Q; ++k)
#pragma unroll
      for (int m = 0; m < NMET; ++m) btile[k][m] = (other[k][m] < best[k][m]) ? t : btile[k][m];
    sweep_tile<Q, NMET>(refs + (t + 1) * kTrk, qx, qy, qz, other, best);
#pragma unroll
    for (int k = 0; k < Q; ++k)
#pragma unroll
      for (int m = 0; m < NMET; ++m) btile[k][m] = (best[k][m] < other[k][m]) ? t + 1 : btile[k][m];
  }
  if (t < ntile) {   // odd number of sub-tiles
    sweep_tile<Q, NMET>(refs + t * kTrk, qx, qy, qz, best, other);
#pragma unroll
    for (int k = 0; k < Q; ++k)
#pragma unroll
      for (int m = 0; m < NMET; ++m) {
        btile[k][m] = (other[k][m] < best[k][m]) ? t : btile[k][m];
        best[k][m] = other[k][m];
      }
  }
}

// Single-metric form of sweep() for metric MET (used by the fused loop's mis-prediction repair): the same expression
// tree per metric (metric_sqdist<MET> == the a0..a3 of the fused form), the same min3 / strict-< bookkeeping, hence
// bit-identical (best, btile) for that metric.
template <int Q, int MET>
__device__ __forceinline__ void sweep_one(const float4* __restrict__ refs, int ntile, const float (&qx)[Q],
                                          const float (&qy)[Q], const float (&qz)[Q], float (&best)[Q], int (&btile)[Q]) {
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    best[k] = INFINITY;
    btile[k] = 0;
  }
  for (int t = 0; t < ntile; ++t) {
    float tm[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) tm[k] = INFINITY;
    const float4* rp = refs + t * kTrk;
#pragma unroll 4
    for (int j = 0; j < kTrk; j += 2) {
      const float4 a = rp[j], c = rp[j + 1];
      asm volatile("" ::"v"(a.w), "v"(c.w));
#pragma unroll
      for (int k = 0; k < Q; ++k)
        tm[k] = min3f(tm[k], metric_sqdist<MET>(a.x - qx[k], a.y - qy[k], a.z - qz[k]),
                      metric_sqdist<MET>(c.x - qx[k], c.y - qy[k], c.z - qz[k]));
    }
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      const bool lt = tm[k] < best[k];
      best[k] = lt ? tm[k] : best[k];
      btile[k] = lt ? t : btile[k];
    }
  }
}

// Sum NV per-thread values over the workgroup into out[0..NV) (LDS).
template <int BLOCK, int NV>
__device__ __forceinline__ void block_sum(float (&v)[NV], float* red, float* out) {
  constexpr int NW = BLOCK / 64;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) red[wave * kAccStride + i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    float a = 0.f;
#pragma unroll
    for (int w = 0; w < NW; ++w) a += red[w * kAccStride + threadIdx.x];
    out[threadIdx.x] = a;
  }
}


// acc = 2 * acc + bit in ONE instruction: v_addc_co_u32 adds the lane's bit of a 64-bit lane mask (the compare's SGPR pair) as
// carry-in.  Replaces v_cndmask + v_or (+ v_min) wherever per-lane bits are collected: box tests, rescans.
__device__ __forceinline__ unsigned shift_in_mask(unsigned acc, unsigned long long lanes) {
  unsigned long long carry_out;
  asm("v_addc_co_u32_e64 %0, %1, %0, %0, %2" : "+v"(acc), "=s"(carry_out) : "s"(lanes));
  return acc;
}
__device__ __forceinline__ unsigned shift_in(unsigned acc, bool bit) { return shift_in_mask(acc, __builtin_amdgcn_ballot_w64(bit)); }

// Exact NN recovery for one query: re-evaluate the winning 16-reference tracking unit (kTrk; half a sub-tile -- the sweeps and the
// pruned walks track the arg-min at this granularity since the end of round 3: half the re-evaluations) with the bit-identical
// expression and return the lowest matching reference.  The scan order is rotated per lane: units are 256 B apart, so an
// un-rotated scan puts all lanes of a ds_read_b128 group on the same LDS bank quad.
// XOR256 (the cloud is 256-B aligned in LDS): lane l reads slot (i ^ (l & 15)) -- 16 distinct slots in each of the instruction's
// 16-lane groups -- and collects the matches as one bit per read (shift_in); the lowest matching index is decoded after the scan
// (one match unless two references tie exactly).  Otherwise: (j + rot) mod 16, min-tracked.
template <int MET, int BATCH, bool XOR256 = false>
__device__ __forceinline__ float4 recover_nn(const float4* __restrict__ rp, float qx, float qy, float qz, float bd, int rot,
                                             int& j_out) {
  int jb = kTrk;
  static_assert(kTrk == 16 && kTrk % BATCH == 0, "one 256-B unit of 16 slots");
  if constexpr (XOR256) {
    const unsigned r16 = (unsigned)rot & 15u;
    const unsigned xa = (unsigned)(size_t)(lds_f4)rp + (r16 << 4);
    unsigned match = 0u;                          // bit (31 - e) = read e matched
#pragma unroll 1
    for (int c = 0; c < kTrk; c += BATCH) {
      float4 r[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const houv_f4v v = *(lds_f4)(size_t)(xa ^ ((unsigned)(c + u) << 4));
        r[u] = make_float4(v.x, v.y, v.z, v.w);
      }
#pragma unroll
      for (int u = 0; u < BATCH; ++u) asm volatile("" ::"v"(r[u].x), "v"(r[u].y), "v"(r[u].z), "v"(r[u].w));   // keep b128
#pragma unroll
      for (int u = 0; u < BATCH; ++u)
        match = shift_in(match, metric_sqdist<MET>(r[u].x - qx, r[u].y - qy, r[u].z - qz) == bd);
    }
    match <<= 32 - kTrk;                          // read e at bit 31 - e
    while (match != 0u) {                         // one round unless references tie (or none: not a point)
      const int e = __clz((int)match);
      match &= ~(0x80000000u >> e);
      jb = min(jb, (int)((unsigned)e ^ r16));
    }
  } else {
#pragma unroll 1
    for (int c = 0; c < kTrk; c += BATCH) {
      float4 r[BATCH];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) r[u] = rp[(c + u + rot) & (kTrk - 1)];
#pragma unroll
      for (int u = 0; u < BATCH; ++u) asm volatile("" ::"v"(r[u].x), "v"(r[u].y), "v"(r[u].z), "v"(r[u].w));   // keep b128
#pragma unroll
      for (int u = 0; u < BATCH; ++u) {
        const float d = metric_sqdist<MET>(r[u].x - qx, r[u].y - qy, r[u].z - qz);
        jb = min(jb, (d == bd) ? ((c + u + rot) & (kTrk - 1)) : kTrk);   // lowest matching index, whatever the order
      }
    }
  }
  j_out = jb & (kTrk - 1);
  return rp[j_out];
}

// ---------------------------------------------------------------------------------------------------------------
// EXACT pruned search (houv_solve_iterate_pruned).  References are grouped in the same 32-point sub-tiles as the brute-force
// sweep; every sub-tile carries an axis-aligned bounding box.  For every query and metric m the distance to the point that
// was its NN in the previous iteration is an upper bound ub[m] that is attained; a sub-tile whose box is farther from the
// query than ub[m] for every metric cannot contain any of its NNs -- nor a point tying with one -- and is skipped.  The
// surviving sub-tiles are visited in ascending order with the same min3 / strict-< bookkeeping as sweep(), so (best, btile)
// come out BIT-IDENTICAL to the brute-force sweep.  A query's list of sub-tiles is one 64-bit mask (<= 64 sub-tiles, i.e.
// clouds of <= 2048 points; super-tiles of two sub-tiles up to 4096).
// ---------------------------------------------------------------------------------------------------------------

// point owned by (thread, k): chunk k of all lanes covers points [k*BLOCK, (k+1)*BLOCK) (strided: coalesced loads)
template <int BLOCK>
__device__ __forceinline__ int pt_index(int k) { return k * BLOCK + tid_x(); }
// the uniform part of pt_index (pt_index(k) = pt_base(k) + thread index): buffer accesses take it as a uniform offset
template <int BLOCK>
constexpr int pt_base(int k) { return k * BLOCK; }

// Remembered nearest neighbours of the pruned search (nn_ws): per direction one record of 4 x int16 per query, the NN index of
// metric m at int16 m, so that the bounds take ONE 8-byte load per query.  `dir_off` = byte offset of the direction's records.
constexpr int kNnRec = 8;

// r = lanes ? b : a per lane, as ONE v_cndmask on a compare's SGPR pair.  Written out because the compiler turns the nested selects
// of the walk's unit bookkeeping into two levels of exec-masked branches (s_and_saveexec + s_cbranch_execz + v_mov per level).
__device__ __forceinline__ unsigned select_mask(unsigned long long lanes, unsigned a, unsigned b) {
  unsigned r;
  asm("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(lanes));
  return r;
}

// Index of the lowest set bit of a 32-bit word, -1 for 0: the bare instruction (the compiler guards __ffs(x) - 1 with a compare and
// a select for the empty word, which v_ffbl_b32 already answers with -1).
__device__ __forceinline__ unsigned lowest_bit_or_m1(unsigned x) {
  unsigned r;
  asm("v_ffbl_b32_e32 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

// Minima of the NMET squared distances between one query and the 32 references of ONE sub-tile, gathered per lane, SEPARATELY for the
// sub-tile's two tracking units (references 0..15 -> ta, 16..31 -> tb).  The lane's sub-tile starts at LDS byte address
// (xa & ~511); the scan order is rotated per lane by XOR over the 16 slots of a 256-B half -- xa carries (lane & 15) << 4 in bits
// 4..7 -- and both halves are read through one address (the second read is an immediate offset: one v_xor per TWO reads); needs the
// clouds 512-B aligned in LDS (solve.hip aligns the dynamic segment); conflict-free as (lane ^ i) % 16 takes 16 distinct slots in
// every ds_read_b128 lane group.  A min3 takes two references of the SAME half, so the two accumulators cost no instruction more
// than one.  The reads are software-pipelined: while a batch of four references is being evaluated the next batch is in flight
// (ping-pong register sets).  The eight batches are written out (no loop): the first min3 of each chain is three-address and takes
// the caller's running minimum `cb` (first unit) or +inf (second unit) as an operand, so neither accumulator is initialised by a
// copy; the slot offsets are immediates; and no prefetch runs past the last batch.  Same expression trees as sweep_tile(); the
// order inside a tracking unit does not matter to a minimum.  ta = min(cb, first unit), tb = min(second unit).
// NaN: v_min3 returns the minimum of its non-NaN operands, so a NaN distance never enters a chain and a chain that starts at a
// number (cb is +inf or a distance, never NaN) ends at a number, as in sweep_tile().
// MSET (walk_variant, houv_math.h): bit m clear = metric m is not evaluated -- no fma of its own, no min3; cb[m], ta[m] and tb[m]
// are neither read nor written, so they take no registers.  The metrics kept have the expression trees of the full set (metric 0
// is still fma(az, az, a3) with a3 = fma(ay, ay, axx), whether metric 3 is kept or not): what is not used is simply not formed.
template <int NMET, int MSET = (1 << NMET) - 1>
__device__ __forceinline__ void gather_tile_min(unsigned xa, float cx, float cy, float cz, const float (&cb)[NMET],
                                                float (&ta)[NMET], float (&tb)[NMET]) {
  constexpr int kBatch = 4, kHalf = kSub / 2;
  static_assert(kSub == 32 && kHalf == kTrk, "two 256-B tracking units of 16 slots");
  auto fetch = [&](float4 (&r)[kBatch], int i0) {
#pragma unroll
    for (int u = 0; u < kBatch; u += 2) {
      lds_f4 p = (lds_f4)(size_t)(xa ^ ((unsigned)((i0 + u / 2) & (kHalf - 1)) << 4));
      const houv_f4v v0 = p[0], v1 = p[kHalf];
      r[u] = make_float4(v0.x, v0.y, v0.z, v0.w);           // first unit
      r[u + 1] = make_float4(v1.x, v1.y, v1.z, v1.w);       // second unit
    }
  };
  auto eval2 = [&](const float4 a, const float4 c, const float (&in)[NMET], float (&t)[NMET]) {   // two references of one unit
    const float ax = a.x - cx, ay = a.y - cy, az = a.z - cz;
    const float bx = c.x - cx, by = c.y - cy, bz = c.z - cz;
    if constexpr (NMET == 4) {
      const float axx = ax * ax, ayy = ay * ay, bxx = bx * bx, byy = by * by;
      const float a3 = __builtin_fmaf(ay, ay, axx), b3 = __builtin_fmaf(by, by, bxx);
      const float a1 = __builtin_fmaf(az, az, ayy), b1 = __builtin_fmaf(bz, bz, byy);
      const float a2 = __builtin_fmaf(az, az, axx), b2 = __builtin_fmaf(bz, bz, bxx);
      const float a0 = __builtin_fmaf(az, az, a3), b0 = __builtin_fmaf(bz, bz, b3);
      if constexpr ((MSET & 1) != 0) t[0] = min3f(in[0], a0, b0);
      if constexpr ((MSET & 2) != 0) t[1] = min3f(in[1], a1, b1);
      if constexpr ((MSET & 4) != 0) t[2] = min3f(in[2], a2, b2);
      if constexpr ((MSET & 8) != 0) t[3] = min3f(in[3], a3, b3);
    } else {
      t[0] = min3f(in[0], metric_sqdist<0>(ax, ay, az), metric_sqdist<0>(bx, by, bz));
    }
  };
  float inf[NMET];
#pragma unroll
  for (int m = 0; m < NMET; ++m) inf[m] = INFINITY;
  auto eval = [&](float4 (&r)[kBatch], bool first) {
#pragma unroll
    for (int u = 0; u < kBatch; ++u) asm volatile("" ::"v"(r[u].x), "v"(r[u].y), "v"(r[u].z), "v"(r[u].w));   // keep b128
    static_assert(kBatch == 4, "a batch = two slots x two units");
    if (first) {
      eval2(r[0], r[2], cb, ta);
      eval2(r[1], r[3], inf, tb);
    } else {
      eval2(r[0], r[2], ta, ta);
      eval2(r[1], r[3], tb, tb);
    }
  };
  // A partial metric set pins the pipeline as written: the address of a batch's reads is made to depend (an empty asm, no
  // instruction) on the evaluation before it.  Left alone, the scheduler fills the arithmetic a dropped metric frees with reads
  // hoisted from later batches, 4 VGPRs each: the three-metric loops took up to 19 VGPRs MORE than the full one and spilled what
  // lives across the walk.  The full set keeps the schedule it had.
  constexpr bool kPin = NMET == 4 && MSET != (1 << NMET) - 1;
  float4 ra[kBatch], rb[kBatch];
  fetch(ra, 0);
#pragma unroll
  for (int i0 = 0; i0 < kHalf; i0 += kBatch) {
    fetch(rb, i0 + kBatch / 2);
    eval(ra, i0 == 0);
    if constexpr (kPin) asm volatile("" : "+v"(xa));
    if (i0 + kBatch < kHalf) fetch(ra, i0 + kBatch);
    eval(rb, false);
    if constexpr (kPin) asm volatile("" : "+v"(xa));
  }
}

// (running minimum, tracking unit) of one query and metric after a sub-tile whose unit minima are ta -- threaded: already
// min(running, first unit) -- and tb (second unit).  Units are taken in ascending order with strict <, as sweep() takes them:
// five instructions, no branch (two compares into SGPR pairs, three selects on them).  A NaN never reaches here (gather_tile_min).
__device__ __forceinline__ void take_units(float ta, float tb, int unit0, float& cb, int& ct) {
  const unsigned long long la = __builtin_amdgcn_ballot_w64(ta < cb), lb = __builtin_amdgcn_ballot_w64(tb < ta);
  ct = (int)select_mask(lb, select_mask(la, (unsigned)ct, (unsigned)unit0), (unsigned)unit0 + 1u);
  cb = __uint_as_float(select_mask(lb, __float_as_uint(ta), __float_as_uint(tb)));
}

// Which sub-tiles each of this lane's queries must visit: the bound per metric is the distance to the point that was the
// query's nearest neighbour in the previous iteration (`prev`, attained), the test a point-to-box distance per metric.
// `need` (workgroup-uniform; term_masks, houv_math.h): bit m clear = this direction's term of metric m provably loses the min
// and is not computed: its bound is -1, so no box passes on its account and the lists shrink.
// MSET (a compile-time superset of `need`; walk_variant, houv_math.h): a metric outside it has no remembered-neighbour distance, no
// box distance, no compare and no OR.  Its verdict was "no box passes" before (bound -1 against a distance >= 0 or NaN), so the
// masks are the same bits.  A metric inside MSET but outside `need` keeps the run-time bound -1.
//
// Group cull (box_test_group, houv_math.h, where the proof is): a wave's 64 queries of one k are 64 consecutive points of a
// k-d-sorted cloud -- two leaves (one super-tile under TS = 1), whose boxes tile_boxes has already formed from the very
// coordinates tested here (`qboxes`; entries past `nqtile` were never written and are left out).  Per k, lane b tests reference
// box b against that group box with the wave's largest bound per metric; the ballot is the 64-bit scalar mask of the boxes that
// ANY query of the group can pass, and the per-query tests run in a scalar loop over its set bits only.  A culled box fails
// every lane's own test, so the visit masks are the bits the full loop over all boxes gave, not a superset.
// `qboxes` of sweep A is sm.mbox, written before the call with no barrier in between: a wave reads only the (up to) two entries
// of its own lanes 0 and 32 for each k, and a wave's LDS accesses complete in order.
// Out: the masks, parked in the .w lanes of wlo / whi at the queries' own indices (low / high word), and their lengths `len`.
// nsurv_out: the boxes that survived, summed over the wave's Q groups (a scalar; pruned_sweep_sorted counts it).
__device__ __forceinline__ unsigned& w_slot(float4* cloud, int q) { return reinterpret_cast<unsigned*>(cloud + q)[3]; }
__device__ __forceinline__ unsigned lane_bit(unsigned long long lanes) {   // 1 in the lanes of a compare's SGPR pair, else 0
  unsigned r;
  asm("v_cndmask_b32_e64 %0, 0, 1, %1" : "=v"(r) : "s"(lanes));
  return r;
}

template <int BLOCK, int Q, int NMET, int MSET = (1 << NMET) - 1, int TS = 0>
__device__ __forceinline__ void prune_masks(const float4* __restrict__ refs, const float4* __restrict__ boxes, int ntile,
                                            const float4* qboxes, int nqtile,
                                            const float (&qx)[Q], const float (&qy)[Q], const float (&qz)[Q],
                                            buf_t ws, int prev_off, int count, unsigned need,
                                            float4* wlo, float4* whi, int (&len)[Q], int& nsurv_out) {
  float ub[Q][NMET];
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const bool ok = pt_index<BLOCK>(k) < count;
    // the query's record (a lane past the end of the cloud keeps index 0: its bounds are discarded below)
    unsigned w0 = 0u, w1 = 0u;
    const int voff = tid_x() * kNnRec, soff = prev_off + pt_base<BLOCK>(k) * kNnRec;
    if (ok) {
      if constexpr (NMET == 4) {
        const auto r = __builtin_amdgcn_raw_buffer_load_b64(ws, voff, soff, 0);
        w0 = r[0]; w1 = r[1];
      } else {
        w0 = __builtin_amdgcn_raw_buffer_load_b32(ws, voff, soff, 0);
      }
    }
    if constexpr ((MSET & 1) != 0) { const float4 r = refs[w0 & 0xffffu]; ub[k][0] = metric_sqdist<0>(r.x - qx[k], r.y - qy[k], r.z - qz[k]); }
    if constexpr (NMET == 4) {
      if constexpr ((MSET & 2) != 0) { const float4 r = refs[w0 >> 16]; ub[k][1] = metric_sqdist<1>(r.x - qx[k], r.y - qy[k], r.z - qz[k]); }
      if constexpr ((MSET & 4) != 0) { const float4 r = refs[w1 & 0xffffu]; ub[k][2] = metric_sqdist<2>(r.x - qx[k], r.y - qy[k], r.z - qz[k]); }
      if constexpr ((MSET & 8) != 0) { const float4 r = refs[w1 >> 16]; ub[k][3] = metric_sqdist<3>(r.x - qx[k], r.y - qy[k], r.z - qz[k]); }
    }
#pragma unroll
    for (int m = 0; m < NMET; ++m)   // box distances are rounded: stay conservative
      if ((MSET >> m) & 1) ub[k][m] = (ok && ((need >> m) & 1u)) ? (ub[k][m] * 1.00001f + 1e-30f) : -1.f;
  }
  // ---- group verdicts: lane b holds reference box b ----
  unsigned long long surv[Q];
  {
    const int bl = tid_x() & 63;
    const bool live = bl < ntile;
    const float4 blo4 = boxes[live ? 2 * bl : 0], bhi4 = boxes[live ? 2 * bl + 1 : 1];
    const float blo[3] = {blo4.x, blo4.y, blo4.z}, bhi[3] = {bhi4.x, bhi4.y, bhi4.z};
    const int wave0 = __builtin_amdgcn_readfirstlane(tid_x()) & ~63;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
      float gub[NMET];
#pragma unroll
      for (int m = 0; m < NMET; ++m) {
        gub[m] = -1.f;
        if ((MSET >> m) & 1) gub[m] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_fmax_to_lane63(ub[k][m])), 63));
      }
      float glo[3] = {INFINITY, INFINITY, INFINITY}, ghi[3] = {-INFINITY, -INFINITY, -INFINITY};
      const int t0 = (pt_base<BLOCK>(k) + wave0) >> (5 + TS);
#pragma unroll
      for (int h = 0; h < 2 - TS; ++h) {
        if (t0 + h < nqtile) {   // wave-uniform
          const float4 l = qboxes[2 * (t0 + h)], u = qboxes[2 * (t0 + h) + 1];
          glo[0] = fminf(glo[0], l.x); glo[1] = fminf(glo[1], l.y); glo[2] = fminf(glo[2], l.z);
          ghi[0] = fmaxf(ghi[0], u.x); ghi[1] = fmaxf(ghi[1], u.y); ghi[2] = fmaxf(ghi[2], u.z);
        }
      }
      surv[k] = __builtin_amdgcn_ballot_w64(live && box_test_group<NMET>(glo, ghi, blo, bhi, gub, (unsigned)MSET));
    }
  }
  unsigned alo[Q], ahi[Q];
#pragma unroll
  for (int k = 0; k < Q; ++k) alo[k] = ahi[k] = 0u;
  // per query and surviving box (18 instructions; wave-uniform box: the reads are LDS broadcasts from a scalar address): the box
  // point nearest to the query is the query clamped into the box (v_med3), its offset squared per axis and summed per metric; the
  // verdict goes to bit `bit` of the word: the lane's 0 / 1 of the OR-ed compares, shifted and OR-ed in one instruction
  auto test = [&](const float4 lo, const float4 hi, int k, int bit, unsigned& acc) {
    const float dx = qx[k] - __builtin_amdgcn_fmed3f(qx[k], lo.x, hi.x);
    const float dy = qy[k] - __builtin_amdgcn_fmed3f(qy[k], lo.y, hi.y);
    const float dz = qz[k] - __builtin_amdgcn_fmed3f(qz[k], lo.z, hi.z);
    unsigned long long in;                              // lane mask of the compares, OR-ed on the scalar unit (no branches)
    if constexpr (NMET == 4) {
      const float xx = dx * dx, yy = dy * dy;
      const float s3 = __builtin_fmaf(dy, dy, xx), s1 = __builtin_fmaf(dz, dz, yy), s2 = __builtin_fmaf(dz, dz, xx);
      const float s0 = __builtin_fmaf(dz, dz, s3);
      in = 0ull;                                        // s3 is still formed where s0 needs it
      if constexpr ((MSET & 1) != 0) in |= __builtin_amdgcn_ballot_w64(s0 <= ub[k][0]);
      if constexpr ((MSET & 2) != 0) in |= __builtin_amdgcn_ballot_w64(s1 <= ub[k][1]);
      if constexpr ((MSET & 4) != 0) in |= __builtin_amdgcn_ballot_w64(s2 <= ub[k][2]);
      if constexpr ((MSET & 8) != 0) in |= __builtin_amdgcn_ballot_w64(s3 <= ub[k][3]);
    } else {
      in = __builtin_amdgcn_ballot_w64(__builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx)) <= ub[k][0]);
    }
    acc |= lane_bit(in) << bit;
  };
  // the set bits of one word of a survivor mask, lowest first (any order would do), scanned on the scalar unit.  The next
  // survivor's box is read while this one is tested (after the last one, that box again: a read for nothing): the reads are
  // issued ahead of the test -- the scheduler moves nothing across the barrier; left alone it sinks them below the test and the
  // loop waits out an LDS round trip per box -- and are first needed, by an empty asm, before the back-edge.  Whole float4s:
  // ds_read_b128 takes half the LDS cycles of ds_read_b96.
  auto run = [&](unsigned w, int t_base, int k, unsigned& acc) {
    if (w == 0u) return;
    int b = __builtin_ctz(w);
    float4 lo = boxes[2 * (t_base + b)], hi = boxes[2 * (t_base + b) + 1];
    for (;;) {
      w &= w - 1u;
      asm volatile("" : "+s"(w));
      const int nb = w != 0u ? __builtin_ctz(w) : b;
      const float4 nlo = boxes[2 * (t_base + nb)], nhi = boxes[2 * (t_base + nb) + 1];
      __builtin_amdgcn_sched_barrier(0);
      test(lo, hi, k, b, acc);
      asm volatile("" ::"v"(nlo.x), "v"(nlo.y), "v"(nlo.z), "v"(nlo.w), "v"(nhi.x), "v"(nhi.y), "v"(nhi.z), "v"(nhi.w));
      if (w == 0u) break;
      b = nb; lo = nlo; hi = nhi;
    }
  };
  int nsurv = 0;
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    run((unsigned)surv[k], 0, k, alo[k]);
    run((unsigned)(surv[k] >> 32), 32, k, ahi[k]);
    nsurv += __popcll(surv[k]);
    // the mask is parked here, in the .w lanes of the two clouds (see pruned_sweep_sorted), inside the code of the metric set:
    // its length alone leaves, not eight mask registers that meet those of the other sets' copies
    len[k] = __popc(alo[k]) + __popc(ahi[k]);
    const int q = pt_index<BLOCK>(k);
    if (q < count) {
      w_slot(wlo, q) = alo[k];
      w_slot(whi, q) = ahi[k];
    }
  }
  nsurv_out = nsurv;
}

// ---------------------------------------------------------------------------------------------------------------
// Pruned sweep, BALANCED form (round 3; solve_kernel<.., PRUNE = 2 / 3>).  Round 2's walk by the owning lanes lost ~20 % of its
// steps to lane imbalance (a wave runs for its longest lane) and ~25 % of its instructions to "which of my lists am I on"
// selects (removed; profiles/r03_ab_walks.txt).  Here the walk is detached from ownership:
//   1. every thread computes the visit masks of ITS queries (prune_masks) and parks them in LDS -- in the .w lanes of the
//      two clouds' float4 slots, which nothing else uses (8 bytes per point index: exactly one 64-bit mask);
//   2. the workgroup's queries are counting-sorted by list length, longest first (65 bins, LDS atomics, 2 bytes per query);
//   3. waves take blocks of 64 consecutive sorted queries from a shared counter (longest blocks first: LPT scheduling); the
//      64 lists of a block have (nearly) the same length, so all lanes walk in lock-step with no idle lanes, the query, its
//      running minima and sub-tile ids in fixed registers (~22 bookkeeping instructions per step instead of ~110); a lane
//      whose list is a step shorter re-evaluates its last sub-tile, which cannot change its result;
//   4. per query the sub-tile ids of the minima go back to the owner through the query's (now consumed) mask slot, the four
//      minima through a per-hypothesis scratch record in global memory (16 bytes per query; L2-resident).
// A query's sub-tiles are still visited in ascending order with strict <, so (best, btile) are bit-identical to sweep().
// LDS cost: 2 bytes per query + 0.5 KB, so two 512-thread workgroups still share a CU (the phases of one hide behind
// the sweeps of the other: a single 1024-thread workgroup per CU measured 14 % slower on the brute-force kernel).
// ---------------------------------------------------------------------------------------------------------------
struct SortedStage {
  unsigned short* order;      // [BLOCK * Q]  query ids, longest list first
  int* hist;                  // [65 + 65 + 2]  bin counts (by 64 - length) | bin bases | next block
};


// wlo / whi: the two LDS clouds (both hold >= count entries); .w of wlo[q] carries the low half of query q's mask and,
// after the walk, the tracking-unit ids (8 bits each: <= 256 units of 16 references) of its minima; .w of whi[q] the high half.
// TS = 1 (clouds of 2049..4096 points): the masks are over 64 SUPER-tiles of two sub-tiles each (`boxes`, `ntile` count
// super-tiles); a visit evaluates both sub-tiles in ascending order, the minima carry tracking-unit ids (0..255) for the rescans.
// `need`: see prune_masks; (best, btile) of a metric whose bit is clear are never read downstream (select_all, park_sqrt_sums,
// park_grad_sums and final_sums skip on `need`): +inf and unit 0 where the walk variant leaves the metric out, the minimum over
// the other metrics' lists where a superset variant computes it.
// Walk variants: `need` is workgroup-uniform, so it selects -- with one scalar table look-up (walk_variant, houv_math.h) and one
// switch each -- box tests and a block loop compiled for the metric set MSET.  The counting sort and the barriers S1..S3 between
// the two are common code: every wave meets the same barriers whichever variant it runs.
// `walk_hist` (houv_debug_set("solve_walk_hist")): 16 counters, +1 in slot `need` per wave and sweep; null = off.
// `qboxes`: the boxes of the QUERY cloud (the other of sm.tbox / sm.mbox), see prune_masks.
// `cull` (houv_debug_set("solve_cull_stats")): four counters, added to once per wave and sweep -- groups tested (Q), boxes
// surviving, per-query tests executed, per-query tests of a loop over all boxes (the last two per lane: 64 a box); null = off.
template <typename F>
__device__ __forceinline__ void walk_dispatch(unsigned mset, F&& f) {
#define HOUV_WALK_CASE(S)                                                          \
  case S:                                                                          \
    if constexpr (walk_instantiated(S)) f(std::integral_constant<int, S>{});       \
    break;
  switch (mset) {   // mset = walk_variant(need): always one of the instantiated sets
    HOUV_WALK_CASE(1) HOUV_WALK_CASE(2) HOUV_WALK_CASE(3) HOUV_WALK_CASE(4) HOUV_WALK_CASE(5) HOUV_WALK_CASE(6) HOUV_WALK_CASE(7)
    HOUV_WALK_CASE(8) HOUV_WALK_CASE(9) HOUV_WALK_CASE(10) HOUV_WALK_CASE(11) HOUV_WALK_CASE(12) HOUV_WALK_CASE(13) HOUV_WALK_CASE(14)
    default: f(std::integral_constant<int, 15>{}); break;
  }
#undef HOUV_WALK_CASE
}

template <int BLOCK, int Q, int NMET, int TS = 0>
__device__ __forceinline__ void pruned_sweep_sorted(const float4* __restrict__ refs, const float4* __restrict__ boxes, int ntile,
                                                    const float4* qboxes, const float4* __restrict__ qarr, float4* wlo, float4* whi,
                                                    const float (&qx)[Q], const float (&qy)[Q], const float (&qz)[Q],
                                                    buf_t ws, int prev_off, int count, unsigned need,
                                                    const SortedStage& st, float4* __restrict__ res, float (&best)[Q][NMET],
                                                    int (&btile)[Q][NMET], unsigned long long* __restrict__ stats,
                                                    unsigned long long* __restrict__ walk_hist,
                                                    unsigned long long* __restrict__ cull) {
  static_assert(BLOCK % 64 == 0 && BLOCK >= 128, "whole waves; thread 64 resets the block counter");
  const int tid = tid_x(), lane = tid & 63;
  const int nqtile = (count + (kSub << TS) - 1) >> (5 + TS);   // boxes of the query cloud that tile_boxes wrote
  int len[Q], rnk[Q];
  int nsurv = 0;
  if constexpr (NMET == 4) {
    walk_dispatch((unsigned)(walk_variant_table() >> (4u * need)) & 15u, [&](auto mset) {
      prune_masks<BLOCK, Q, NMET, decltype(mset)::value, TS>(refs, boxes, ntile, qboxes, nqtile, qx, qy, qz, ws, prev_off, count, need,
                                                             wlo, whi, len, nsurv);
    });
  } else {
    prune_masks<BLOCK, Q, NMET, 1, TS>(refs, boxes, ntile, qboxes, nqtile, qx, qy, qz, ws, prev_off, count, need, wlo, whi,
                                       len, nsurv);
  }
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    rnk[k] = 0;
    if (pt_index<BLOCK>(k) < count) rnk[k] = atomicAdd(&st.hist[64 - len[k]], 1);   // place inside its bin (any order: results do not depend on it)
  }
  // barrier S1 -- writers: every thread's bin atomics above; readers: every wave's bin scan below.  It also orders the previous
  // walk's last block-counter atomics (all before barrier S3 of that sweep) against the counter's reset here.
  __syncthreads();
  // Exclusive prefix over the 65 bins, by EVERY wave for itself (one LDS read per lane + a DPP scan; lane b holds bin b's base and
  // a query fetches its own with one ds_bpermute): no wave waits for another to publish the bases, which took a barrier of its own.
  // Bin 64 = empty lists (a query none of whose box tests passes: a NaN coordinate) starts where bin 63 ends.
  const int bin_c = st.hist[lane];
  const int bin_incl = wave_incl_scan_dpp(bin_c);
  const int base64 = __builtin_amdgcn_readlane(bin_incl, 63);
  if (tid == 64) st.hist[130] = 0;                            // next block
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int q = pt_index<BLOCK>(k);
    const int bin = 64 - len[k];
    const int base = __builtin_amdgcn_ds_bpermute((bin & 63) << 2, bin_incl - bin_c);
    if (q < count) st.order[(bin == 64 ? base64 : base) + rnk[k]] = (unsigned short)q;
  }
  // barrier S2 -- writers: the order entries and mask slots of every thread, the counter reset; readers: the walk of every wave.
  // Every wave has also read the bins by now, so one wave clears them for the next sweep (whose atomics come after barrier S3).
  __syncthreads();
  if (tid < 65) st.hist[tid] = 0;
  const int nblk = (count + 63) >> 6;
  int asked = 0, nsteps = 0;
  auto walk_blocks = [&](auto mset) {
    constexpr int MSET = decltype(mset)::value;
    for (;;) {
      int b = 0;
      if (lane == 0) b = atomicAdd(&st.hist[130], 1);
      b = __builtin_amdgcn_readfirstlane(b);
      if (b >= nblk) break;
      const int e = b * 64 + lane;
      const bool valid = e < count;                                       // the last block may be partly filled
      const int q = st.order[valid ? e : count - 1];
      unsigned long long mm = valid ? (((unsigned long long)w_slot(whi, q) << 32) | w_slot(wlo, q)) : 0ull;
      const int cap = __builtin_amdgcn_readfirstlane(__popcll(mm));      // sorted: lane 0 holds the block's longest list
      const float4 qp = qarr[q];
      float cb[NMET];
      int ct[NMET];
#pragma unroll
      for (int m = 0; m < NMET; ++m) { cb[m] = INFINITY; ct[m] = 0; }
      asked += __popcll(mm);
      nsteps += cap;
      // the lane's rotated base address, kept across the steps: a step forms its sub-tile's address with one shift-add
      // (from the opaque thread index, like everything else the iteration loop derives per lane: see tid_x)
      const unsigned xbase = (unsigned)(size_t)(lds_f4)refs + (((unsigned)tid_x() & 15u) << 4);
      int t = 0;
#pragma unroll 1
      for (int s = 0; s < cap; ++s) {
        // next sub-tile = lowest set bit, found on the 32-bit halves: v_ffbl gives -1 for an empty word, so the lower of
        // (lo, 32 | hi) as unsigned is the next sub-tile, or -1 for an empty list, which the signed max with t turns into "stay"
        // (lists ascend: the next sub-tile is above t, and the first one is >= 0 = t).  No 64-bit compare, no select.
        const unsigned nxt = min(lowest_bit_or_m1((unsigned)mm), lowest_bit_or_m1((unsigned)(mm >> 32)) | 32u);
        t = max(t, (int)nxt);
        mm &= mm - 1ull;                                                  // 0 stays 0
#pragma unroll
        for (int h = 0; h < (1 << TS); ++h) {
          const int ts = (t << TS) | h;                                   // sub-tile
          const unsigned xa = xbase + (unsigned)ts * (kSub * 16u);
          float ta[NMET], tb[NMET];                                       // ta: the running minima threaded through the first tracking unit
          gather_tile_min<NMET, MSET>(xa, qp.x, qp.y, qp.z, cb, ta, tb);
#pragma unroll
          for (int m = 0; m < NMET; ++m)
            if ((MSET >> m) & 1) take_units(ta[m], tb[m], 2 * ts, cb[m], ct[m]);
        }
      }
      if (valid) {   // a metric outside MSET goes back as it was initialised: +inf, unit 0
        if constexpr (NMET == 4) {
          res[q] = make_float4(cb[0], cb[1], cb[2], cb[3]);
          w_slot(wlo, q) = (unsigned)ct[0] | ((unsigned)ct[1] << 8) | ((unsigned)ct[2] << 16) | ((unsigned)ct[3] << 24);
        } else {
          res[q].x = cb[0];
          w_slot(wlo, q) = (unsigned)ct[0];
        }
      }
    }
  };
  if constexpr (NMET == 4) walk_dispatch((unsigned)(walk_variant_table() >> (4u * need)) & 15u, walk_blocks);
  else walk_blocks(std::integral_constant<int, 1>{});
  if (walk_hist && lane == 0) atomicAdd(&walk_hist[need & 15u], 1ull);   // the unit of stats[2]
  if (cull && lane == 0) {
    nsurv = __builtin_amdgcn_readfirstlane(nsurv);
    asm volatile("" : "+s"(ntile));   // the product below is formed here, not kept in registers around the iteration loop
    atomicAdd(&cull[0], (unsigned long long)Q);
    atomicAdd(&cull[1], (unsigned long long)nsurv);
    atomicAdd(&cull[2], 64ull * (unsigned long long)nsurv);
    atomicAdd(&cull[3], 64ull * (unsigned long long)(Q * ntile));
  }
  if (stats) {
    asked = wave_incl_scan_dpp(asked);
    if (lane == 63) atomicAdd(&stats[0], (unsigned long long)asked);
    if (lane == 0) {
      atomicAdd(&stats[1], (unsigned long long)nsteps);
      atomicAdd(&stats[2], 1ull);                                       // one wave-sweep = 64 x Q queries
    }
  }
  // barrier S3 -- writers: the walk's minima (global; the workgroup's waves share one L1) and unit ids (mask slots) of every
  // wave; readers: the owning lanes below
  __syncthreads();
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    const int q = pt_index<BLOCK>(k);
    const bool ok = q < count && len[k] > 0;                            // padding queries were never walked
    const int qq = ok ? q : 0;
    const unsigned tl = w_slot(wlo, qq);
    if constexpr (NMET == 4) {
      const float4 r = res[qq];
      best[k][0] = ok ? r.x : INFINITY; best[k][1] = ok ? r.y : INFINITY; best[k][2] = ok ? r.z : INFINITY; best[k][3] = ok ? r.w : INFINITY;
      btile[k][0] = ok ? (int)(tl & 255u) : 0; btile[k][1] = ok ? (int)((tl >> 8) & 255u) : 0;
      btile[k][2] = ok ? (int)((tl >> 16) & 255u) : 0; btile[k][3] = ok ? (int)(tl >> 24) : 0;
    } else {
      const float r = res[qq].x;
      best[k][0] = ok ? r : INFINITY;
      btile[k][0] = ok ? (int)(tl & 255u) : 0;
    }
  }
}

// Axis-aligned boxes of the 32-point sub-tiles of a cloud whose points live in this lane's registers (ownership as
// pt_index): within a chunk a sub-tile spans 32 consecutive lanes; a few xor-shuffles reduce it.  box[2t] = lo, box[2t+1] = hi.
// TS = 1: boxes of SUPER-tiles of 64 points (two sub-tiles: a whole wave) instead of sub-tiles.
template <int BLOCK, int Q, int TS = 0>
__device__ __forceinline__ void tile_boxes(const float (&x)[Q], const float (&y)[Q], const float (&z)[Q], int count,
                                           int ntile, float4* __restrict__ box) {
  constexpr int kTile = kSub << TS;
  static_assert(kTile <= 64, "a tile's owners must sit in one wave");
  // xor-shuffle over the tile's lanes, the partner's address formed here from the opaque thread index: __shfl_xor's (from the
  // lane id) were hoisted out of the iteration loop, one VGPR per offset held for the whole kernel
  const int lane4 = tid_x() << 2;
  auto shfl_xor = [&](float v, int o) { return __int_as_float(__builtin_amdgcn_ds_bpermute((lane4 ^ (o << 2)) & 252, __float_as_int(v))); };
#pragma unroll
  for (int k = 0; k < Q; ++k) {
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    if (pt_index<BLOCK>(k) < count) {
      lx = fminf(lx, x[k]); ly = fminf(ly, y[k]); lz = fminf(lz, z[k]);
      hx = fmaxf(hx, x[k]); hy = fmaxf(hy, y[k]); hz = fmaxf(hz, z[k]);
    }
#pragma unroll
    for (int o = 1; o < kTile; o <<= 1) {
      lx = fminf(lx, shfl_xor(lx, o)); ly = fminf(ly, shfl_xor(ly, o)); lz = fminf(lz, shfl_xor(lz, o));
      hx = fmaxf(hx, shfl_xor(hx, o)); hy = fmaxf(hy, shfl_xor(hy, o)); hz = fmaxf(hz, shfl_xor(hz, o));
    }
    const int t = pt_index<BLOCK>(k) / kTile;
    if ((tid_x() % kTile) == 0 && t < ntile) {
      box[2 * t] = make_float4(lx, ly, lz, 0.f);
      box[2 * t + 1] = make_float4(hx, hy, hz, 0.f);
    }
  }
}

}  // namespace houv
