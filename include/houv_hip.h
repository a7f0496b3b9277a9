/* houv_hip.h -- C ABI of libhouv_hip.so: the MI355X (gfx950) HOUV registration hot path.
 *
 * This is the drop-in boundary.  Every entry point replaces one interface of the reference
 * (Dizzy-cell/HOUV; paths relative to the reference root) and keeps its conventions:
 *   - the CALLER allocates every buffer; nothing is allocated or freed in here;
 *   - all pointers are DEVICE pointers to contiguous row-major arrays (fp32 / int32 / fp64 as
 *     declared) on the current device, unless a parameter says "host";
 *   - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the null stream) and
 *     the call returns without synchronising;
 *   - return value 1 = enqueued OK, 0 = error (message via houv_last_error()); this is the
 *     reference's own convention (utils/metrics/CD/chamfer3D/chamfer3D.cu:145-153).
 *
 * No torch types appear in any signature.
 */
#ifndef HOUV_HIP_H_
#define HOUV_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HOUV_ABI_VERSION 2

/* ABI version of the loaded library (== HOUV_ABI_VERSION). */
int houv_abi_version(void);

/* Thread-local text of the last error returned by any call below ("" if none). */
const char* houv_last_error(void);

/* sha256 (first 16 hex digits) of the sources this library was built from (houv_amd/csrc/Makefile): lets a committed
 * profile say which build it measured.  No counterpart in the reference. */
const char* houv_build_id(void);

/* Diagnostic switches for tests, A/B scripts and bench.py (process-wide; never read from the environment).  Names and
 * meanings: houv_amd/csrc/houv_common.h `DebugKnobs`.  Results do not depend on any of them except the ones that select
 * an alternative kernel of the same result for timing.  Returns 0 on an unknown name / out-of-range value.
 * No counterpart in the reference. */
int houv_debug_set(const char* name, long long value);

/* ---------------------------------------------------------------------------------------------
 * Chamfer nearest-neighbour op.
 * Replaces: pybind `chamfer_3D.forward` -> chamfer_cuda_forward
 *           (utils/metrics/CD/chamfer3D/chamfer_cuda.cpp:17-19,31; chamfer3D.cu:136-154; kernel :12-134).
 *   dist1[b,i] = min_j |xyz1[b,i]-xyz2[b,j]|^2   idx1[b,i] = argmin_j (lowest j on ties)
 *   dist2[b,j] = min_i |xyz2[b,j]-xyz1[b,i]|^2   idx2[b,j] = argmin_i
 * fp32 direct-difference arithmetic d = fma(dz,dz,fma(dy,dy,dx*dx)).
 * xyz1[B,N,3] xyz2[B,M,3] dist1[B,N] dist2[B,M] idx1[B,N] idx2[B,M].  N or M == 0 is an error. */
int houv_chamfer_forward(const float* xyz1, const float* xyz2, int B, int N, int M,
                         float* dist1, float* dist2, int32_t* idx1, int32_t* idx2, void* stream);

/* Replaces: pybind `chamfer_3D.backward` -> chamfer_cuda_backward
 *           (chamfer_cuda.cpp:22-26,32; chamfer3D.cu:176-195; kernel :155-174).
 * ACCUMULATES into gradxyz1[B,N,3] / gradxyz2[B,M,3], which the caller must have zero-filled
 * (dist_chamfer_3D.py:56-60), exactly like the reference:
 *   g = 2*graddist1[b,i]; gradxyz1[b,i] += g (x1_i - x2_idx1);  gradxyz2[b,idx1] -= same;  and symmetrically. */
int houv_chamfer_backward(const float* xyz1, const float* xyz2, int B, int N, int M,
                          const float* graddist1, const float* graddist2,
                          const int32_t* idx1, const int32_t* idx2,
                          float* gradxyz1, float* gradxyz2, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Kabsch rigid solve: 3x3 (weighted) covariance reduction + register-resident Jacobi SVD.
 * Replaces: SVDHead.forward (registration/model_utils.py:220-255).
 *   src, corr: [B,3,N] (channel-major like the reference); w: [B,1,N] or NULL.
 *   R[B,3,3], t[B,3].  Centres by the UNWEIGHTED means; reflection fix on det<0. */
int houv_kabsch(const float* src, const float* corr, const float* w_or_null, int B, int N,
                float* R, float* t, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Fused HOUV optimisation loop.
 * Replaces the body of predict_model (registration/models/houv.py:106-138) and of getPredict_angle
 * (registration/train_utils.py:359-456): for every hypothesis (pair p, restart k) it runs
 * `n_iters` x { pose from the 8 unconstrained scalars -> move the source cloud -> robust Chamfer
 * loss (Predict_loss, houv.py:209-222) -> closed-form gradient -> Adam step } entirely on chip.
 *
 *   src[P,N,3], tgt[P,M,3]   the P pairs (NOT replicated K times)
 *   state[P*K,24] fp64       per hypothesis: param[8] = (V0,V1,V2, a, c0,c1,c2, s), adam_m[8], adam_v[8];
 *                            in/out.  With f64_params == 0 the values are fp32 numbers stored widened.
 *   steps_done               Adam steps already applied to `state` (0 for a fresh stage)
 *   n_iters                  iterations to run now (>= 1)
 *   angle_base               0..3: rotation-angle window base*45deg .. base*45+45deg (houv.py:96)
 *   trans_mode               0: sigma = sin(s pi)/8 + 1/8 (houv.py:99)   1: sigma = sin(s pi) (train_utils.py:404)
 *   use_views                1: loss = 6 min_1 + three projected Chamfer terms (houv.py:222)
 *                            0: loss = 6 min_1 (train_utils.py:433)
 *   f64_params               0: fp32 parameters + fp32 Adam (HOUV module)   1: fp64 leaves + fp64 Adam (`solve` twin)
 *   k_full, k_view           top-k sizes: int(N*0.5) and int(N*1) (model_utils_completion.py:85-86)
 *   lr, beta1, beta2, eps    Adam hyper-parameters
 *   loss_scale               d(objective)/d(per-hypothesis loss) = 1/(P*K) for `.mean()` (houv.py:124)
 * Outputs (each may be NULL), all from the LAST forward pass, i.e. before the last Adam step
 * (houv.py:134-136):
 *   out_score[P*K] = min_1   out_loss[P*K]   out_R[P*K,9]   out_T[P*K,3]
 *   out_grad[P*K,8]  d(objective)/d(param) of the last forward
 *   out_cd[P*K,8]    the 8 Chamfer terms: metric m (0 = full, 1..3 = view dropping x,y,z) x
 *                    direction (0: over target points, 1: over moved points) at [2*m+dir]
 * Limits: (roundup32(N)+roundup32(M))*16 B + 8 KiB must fit in 160 KiB of LDS; K >= 1. */
int houv_solve_iterate(const float* src, const float* tgt, int P, int N, int M, int K,
                       double* state, int steps_done, int n_iters,
                       int angle_base, int trans_mode, int use_views, int f64_params,
                       int k_full, int k_view,
                       double lr, double beta1, double beta2, double eps, float loss_scale,
                       float* out_score, float* out_loss, float* out_R, float* out_T,
                       float* out_grad, float* out_cd, void* stream);

/* EXACT accelerated form of houv_solve_iterate (same arguments, same search result; what houv_amd.solver runs by default): every
 * query remembers its nearest neighbour of an earlier iteration; the distance to that point is an
 * attained upper bound, and 32-point sub-tiles whose bounding box lies farther than the bound for all metrics are
 * skipped.  Works best on spatially sorted clouds (houv_amd.solver reorders them so that runs of 32 points are k-d-tree leaves).  The search result
 * and the summation order are those of houv_solve_iterate: same outputs BIT FOR BIT when given the same clouds.
 *   nn_ws[P*K, 16, ws_stride] int16  workspace, in/out, opaque to the caller: per hypothesis rows 0..7 hold the previous
 *              nearest-neighbour indices of every point (one 4 x int16 record per point and direction), rows 8..15 are
 *              scratch (ws_stride x 16 bytes); ws_stride >= max(N, M) and a multiple of 8; nn_ws 16-byte aligned
 *   ws_valid   0: nn_ws holds nothing yet (the first iteration of this call runs the brute-force sweep)
 *              1: nn_ws was left by the previous call on the same hypotheses (chunked launches)
 *             -1: verification mode: every iteration runs the brute-force sweep (nn_ws is not used)
 * Limits: as houv_solve_iterate (N, M <= 4096).  Up to 256 points the brute-force kernel runs (nothing to prune); up to 2048 points
 * a visit mask has one bit per 32-point sub-tile, above one bit per pair of sub-tiles. */
int houv_solve_iterate_pruned(const float* src, const float* tgt, int P, int N, int M, int K,
                              double* state, int steps_done, int n_iters,
                              int angle_base, int trans_mode, int use_views, int f64_params,
                              int k_full, int k_view,
                              double lr, double beta1, double beta2, double eps, float loss_scale,
                              float* out_score, float* out_loss, float* out_R, float* out_T,
                              float* out_grad, float* out_cd,
                              int16_t* nn_ws, int ws_valid, int ws_stride, void* stream);

/* A whole STAGE of the fused loop in one launch (what houv_amd.solver runs for a stage): the arguments of houv_solve_iterate /
 * houv_solve_iterate_pruned, with n_iters the whole stage, plus
 *   chunk_iters        length of an item in iterations (>= 1; the stage's last item may be shorter)
 *   sched_ws[4 + P*K]  int32 scheduling workspace on the device, 4-byte aligned, one per stage in flight; the call zeroes it
 *                      on `stream`.  [0] ticket counter, [1] status, [2..3] spare, [4 + h] chunks of hypothesis h finished.
 * A persistent grid -- as many workgroups as the chip holds at once, at most P*K -- draws tickets from sched_ws[0]; ticket t is
 * the item (chunk t / (P*K), hypothesis t % (P*K)), so a stage has one tail of one item and no part of the chip waits for
 * another.  An item is exactly what houv_solve_iterate[_pruned] does for one hypothesis in a launch of chunk_iters iterations at
 * steps_done + chunk * chunk_iters (pruned: ws_valid || chunk > 0): state, outputs and nn_ws are BIT FOR BIT those of separate
 * launches of chunk_iters.  The out_* values are stored on the stage's last iteration only.
 * Status: a workgroup that starts chunk c > 0 of a hypothesis checks that chunk c - 1 is finished, and waits where it is still
 * running; the wait is bounded by time, and a wait that runs out sets sched_ws[1] non-zero and ends the launch early -- the
 * caller reads sched_ws[1] after synchronising and must treat non-zero as a failed stage.
 * Returns 1 at once when P == 0; 0 with houv_last_error() set when chunk_iters < 1, sched_ws is null or misaligned, or a check of
 * houv_solve_iterate[_pruned] fails.  houv_debug_set("solve_max_workgroups", n) caps the grid (0 = off; tests);
 * houv_debug_set("solve_sched", address of 32 uint64 on the device) collects per XCD: items run, sum of its workgroups' durations,
 * earliest start and latest end in 100-MHz ticks (the caller presets the minima to all ones).  No counterpart in the reference. */
int houv_solve_stage(const float* src, const float* tgt, int P, int N, int M, int K,
                     double* state, int steps_done, int n_iters,
                     int angle_base, int trans_mode, int use_views, int f64_params,
                     int k_full, int k_view,
                     double lr, double beta1, double beta2, double eps, float loss_scale,
                     float* out_score, float* out_loss, float* out_R, float* out_T,
                     float* out_grad, float* out_cd,
                     int chunk_iters, int32_t* sched_ws, void* stream);
int houv_solve_stage_pruned(const float* src, const float* tgt, int P, int N, int M, int K,
                            double* state, int steps_done, int n_iters,
                            int angle_base, int trans_mode, int use_views, int f64_params,
                            int k_full, int k_view,
                            double lr, double beta1, double beta2, double eps, float loss_scale,
                            float* out_score, float* out_loss, float* out_R, float* out_T,
                            float* out_grad, float* out_cd,
                            int16_t* nn_ws, int ws_valid, int ws_stride,
                            int chunk_iters, int32_t* sched_ws, void* stream);

/* First-guess neighbour records for the pruned solve: after this call a stage may start with ws_valid = 1, so that its first
 * iteration runs the pruned search instead of the brute-force sweep.  Any in-range record whose reference lies at a finite
 * distance is an attained bound, so the solve's results do not depend on the guess -- only the length of the first visit lists does.
 * One workgroup per hypothesis: the pose of state[h, 0:8] (fp32, as the solve's prologue forms it) moves the source cloud; both
 * clouds get the boxes of their 32-point runs (a last, partly filled run from its existing points); then, for both directions,
 * every query and every metric in use (metric 0 alone without views) takes the run whose box is nearest to the query in that
 * metric's projection (the query clamped into the box; the lowest run wins ties), and of that run the point nearest in that metric
 * (the lowest index wins ties; strict < from +inf, so a NaN distance never wins).  A query whose chosen run holds no reference at
 * a finite distance takes the first reference of the whole cloud at a finite distance, and 0 when there is none (a NaN query).
 * The records go where the solve reads them: per hypothesis 4 x int16 per query at byte q * 8, metric m at int16 m; direction B
 * (queries = target points, indices into the source order) from byte 0, direction A (queries = moved points, indices into the
 * target) from byte ws_stride * 8.  Rows 8..15 of the workspace, and the int16 of metrics not in use, are left as they are.
 * Every index written is in [0, count) of the cloud it points into.
 * Limits: 257 <= max(N, M) <= 4096 (the sizes the pruned kernels serve); nn_ws non-null and 16-byte aligned; ws_stride >= max(N, M)
 * and a multiple of 8; angle_base 0..3, trans_mode 0..1.  Returns 1 at once when P == 0; 0 with houv_last_error() set, launching
 * nothing, when a check fails.  No counterpart in the reference. */
int houv_solve_seed(const float* src, const float* tgt, int P, int N, int M, int K, const double* state,
                    int angle_base, int trans_mode, int use_views, int16_t* nn_ws, int ws_stride, void* stream);

/* Fused loop for LARGE clouds (what houv_amd.solver runs for 4097..16384 points): the same arguments, outputs and arithmetic
 * contract as houv_solve_iterate, for clouds that do not fit in LDS.  Neither cloud is resident: every workgroup (1024 threads,
 * one hypothesis) holds 4096 query points at a time in registers and streams the other cloud through a double-buffered LDS
 * tile (2 x 1024 points x 16 B); per query only the full metric's minimum and nearest-neighbour unit are kept (6 B of LDS) for
 * its top-k.  LDS per workgroup: 40048 + 6 * max(N, M) bytes (135 KiB at 16384 points); no scratch; one workgroup per CU.
 * Brute force: 2 N M point pairs per hypothesis-iteration -- bound the work per call (houv_amd.solver splits calls along
 * iterations and pairs).  Same search result as houv_solve_iterate; the sums are grouped differently, so outputs agree to
 * fp32 rounding, not bit for bit.  Deterministic, and chunking along iterations (steps_done) is bit-neutral.
 * Limits: 1 <= N, M <= HOUV_LARGE_MAX_POINTS; with use_views, N == M and k_view == N (the reference's loss_view raises
 * otherwise); 1 <= k_full <= min(N, M).  Returns 0 with houv_last_error() set, launching nothing, when a check fails.
 * Order of the checks: the size range and the view rule above first, then the checks houv_solve_iterate makes, in its order:
 * bad argument, P == 0 (returns 1 at once, before the pointers and k_full are looked at), null pointer, top-k range, too
 * many hypotheses.  So a call with both a null pointer and a bad k_full reports the null pointer, and a call that breaks the
 * view rule and also has a bad argument (K <= 0, n_iters <= 0, steps_done < 0, angle_base or trans_mode out of range) reports
 * the view rule. */
#define HOUV_LARGE_MAX_POINTS 16384
int houv_solve_iterate_large(const float* src, const float* tgt, int P, int N, int M, int K,
                             double* state, int steps_done, int n_iters,
                             int angle_base, int trans_mode, int use_views, int f64_params,
                             int k_full, int k_view,
                             double lr, double beta1, double beta2, double eps, float loss_scale,
                             float* out_score, float* out_loss, float* out_R, float* out_T,
                             float* out_grad, float* out_cd, void* stream);

/* Which kernel variant the two entry points above launch for clouds of N and M points (host-only query, no GPU work):
 * *block = threads per workgroup (256 / 512 / 1024), *points_per_lane = query points a lane owns (1..4), *prune_mode =
 * 0 brute-force sweep, 2 / 3 pruned search with the balanced (sorted-block) walk over 32-point sub-tiles / 64-point super-tiles --
 * the template arguments of houv::solve_kernel<block, points_per_lane, metrics, prune_mode>.  Any out pointer may be NULL.
 * Returns 0 with houv_last_error() set when no variant serves the size (max(N,M) > 4096).
 * No counterpart in the reference (its kernel has one fixed launch shape, chamfer3D.cu:142-143); exported so that
 * the test-suite can prove that every variant is compared with the CPU oracle. */
int houv_solve_variant(int N, int M, int pruned, int* block, int* points_per_lane, int* prune_mode);

/* Bytes of LDS one workgroup of that variant reserves (host-only query, no GPU work), -1 with houv_last_error() set when no
 * variant serves the size.  Exported so that the test-suite can assert that two workgroups of the 512-thread pruned kernel
 * still share a CU's 160 KiB. */
long long houv_solve_lds_bytes(int N, int M, int pruned);

/* The pruned four-metric kernels compile their box tests and their walk for a few metric sets only.  `need` (0..15, bit m = this
 * direction's Chamfer term of metric m is computed in this iteration) runs on the returned set: a superset of `need`, 15 = all
 * four metrics (host-only query, no GPU work; -1 with houv_last_error() set for a mask outside 0..15).  Results do not depend on
 * the table.  houv_debug_set("solve_walk_hist", address of 16 uint64 on the device) counts the masks the walks see;
 * houv_debug_set("solve_cull_stats", address of 4 uint64 on the device) counts what the group cull of the box tests did: groups
 * tested, boxes surviving, per-query tests executed, per-query tests of a loop over all boxes.
 * No counterpart in the reference; exported so that the test-suite can prove that every compiled set is exercised. */
int houv_solve_walk_variant(int need);

/* The point order houv_solve_iterate_pruned wants, on the device: every cloud reordered so that consecutive runs of `leaf` points
 * are the leaves of a balanced k-d tree -- bit for bit the permutation of houv_amd.solver.kd_sort (torch) on the same device.
 * Lexicographic (x, y, z) start; then, level by level, every range of more than one tile (tiles = ceil(len / leaf)) is cut at
 * a + (tiles - tiles/2) * leaf and stably reordered along one axis.  rule 0 = "area": the axis whose halves have the smallest
 * summed projected box areas (axis 0 unless a later one is strictly smaller); 1 = "extent": the first axis of the largest
 * max - min.  Floats order as torch's stable GPU sort does: -0 == +0, a NaN by its bits (positive above +Inf, negative below -Inf).
 * Use leaf 32 when max(N, M) <= 2048 and 64 above (houv_amd.solver.sort_leaf), for both clouds, then call the pruned solve.
 *   xyz[P,N,3] -> out[P,N,3] in that order; order_or_null[P,N] int32 = source index of each output point.
 * 1 <= N <= 4096, leaf >= 1, P >= 0; out (and order) must not overlap xyz.  One workgroup per cloud.
 * No counterpart in the reference (its solve takes the clouds as they come). */
int houv_kd_sort(const float* xyz, int P, int N, int leaf, int rule, float* out, int32_t* order_or_null, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Point-to-point ICP refinement, one pair per workgroup (BASELINE configs[3]).
 * Replaces: the per-pair Open3D call of registration/train_ICP.py:137-153
 *   o3d.registration.registration_icp(pcd, pcd2, threshold=0.02, trans_init,
 *       TransformationEstimationPointToPoint(), ICPConvergenceCriteria(max_iteration=500))
 * (open3d==0.9.0, not under /root/reference: its published algorithm is restated; parity unpinned).
 *   src[P,N,3], tgt[P,M,3]; init [P,16] row-major 4x4 or NULL (identity)
 *   max_correspondence_distance: a source point corresponds to its NN in tgt iff dist < this
 *   relative_fitness / relative_rmse: Open3D's ICPConvergenceCriteria defaults are 1e-6 / 1e-6
 * Outputs: out_T[P,16] row-major 4x4 (bottom row 0,0,0,1; maps src into tgt's frame),
 *   out_fitness[P] = #correspondences/N, out_rmse[P] = inlier RMSE, out_iters[P] = updates applied (each may be NULL
 *   except out_T). */
int houv_icp_refine(const float* src, const float* tgt, int P, int N, int M, const float* init_or_null,
                    float max_correspondence_distance, int max_iteration, float relative_fitness,
                    float relative_rmse, float* out_T, float* out_fitness, float* out_rmse, int32_t* out_iters,
                    void* stream);

/* ---------------------------------------------------------------------------------------------
 * DCP feature head building blocks (BASELINE configs[4]): registration/models/dcp.py in fp32,
 * inference (eval-mode BatchNorm folded into per-channel scale/shift by the caller).  The model-level forward
 * (DGCNN -> Transformer -> soft correspondences -> houv_kabsch) is composed from these in houv_amd/models/dcp.py.
 * Layout convention: activations are row-major [rows, channels] ("token-major"), clouds [B,N,3]. */

/* dcp.py:35-42 `knn`: idx[B,N,k] = the k nearest points of xyz[B,N,3] to each point, nearest first, self included.
 * k in {1,3,8,16,20}. */
int houv_knn(const float* xyz, int B, int N, int k, int32_t* idx, void* stream);

/* dcp.py:44-66 + :285: edge feature cat(neighbour, centre)[6] -> relu(scale*(W[64,6] f) + shift) for every (point, neighbour):
 * out[(B*N*k), 64]. */
int houv_edgeconv1(const float* xyz, const int32_t* idx, int B, int N, int k, const float* W, const float* scale,
                   const float* shift, float* out, void* stream);

/* dcp.py:287/290/293/296 `x.max(dim=-1)`: out[p*ldo + c] = max_j act[(p*k+j)*C + c], p < npts (C, ldo multiples of 4).
 * act and out (the first written column) must be 16-byte aligned: the kernel moves four floats at a time. */
int houv_max_over_k(const float* act, long long npts, int k, int C, float* out, int ldo, void* stream);

/* fp32 GEMM on the matrix pipe with fused epilogue (1x1 conv / nn.Linear / attention products):
 *   C = relu?( (alpha * A[M,K] op(B)) * scale[n] + shift[n] + residual[m,n] ),  trans_b=1: B is [N,K] (C = A B^T), 0: [K,N].
 * Batched over outer*inner problems with element strides (s?o, s?i).  scale/shift/residual may be NULL.
 * fp32 in, fp32 out, fp32-grade products: full, 16-byte aligned [N,K] tiles run on the bf16 MFMAs with every operand split into
 * three bf16 parts and six part products per product (error at or below the fp32-input MFMA kernel's, which serves every other
 * shape); an Inf operand yields NaN there.  houv_debug_set("gemm_split", 0) selects the fp32-input kernel everywhere. */
int houv_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, int lda, int ldb, int ldc,
                  int trans_b, int outer, int inner, long long sAo, long long sAi, long long sBo, long long sBi,
                  long long sCo, long long sCi, float alpha, const float* scale_or_null, const float* shift_or_null,
                  const float* residual_or_null, int ldr, long long sRo, long long sRi, int relu, void* stream);

/* dcp.py:26-32 `attention` of MultiHeadedAttention (:198-229), fused: O = softmax(Q K^T * scale) V per (pair, head); the
 * [Nq,Nk] scores stay on chip (online softmax).  Token-major operands: head h of row n of pair p starts at
 * X + p*sX + n*ldX + h*dk.  dk must be 128 (DCP: 512 / 4 heads); strides multiples of 4 floats, pointers 16-byte aligned.
 * Full tiles (Nq % 128 == 0, Nk % 32 == 0) run on the bf16 MFMAs with three-part operand splits (fp32-grade, as houv_gemm_f32) and
 * take a stream-ordered workspace of 12 * P * H * Nk * 128 bytes (hipMallocAsync / hipFreeAsync on `stream`; without it, or with
 * houv_debug_set("attn_split", 0), the fp32-input kernel runs). */
int houv_attention_f32(const float* Q, const float* K, const float* V, float* O, int P, int H, int Nq, int Nk, int dk,
                       int ldq, int ldk, int ldv, int ldo, long long sQ, long long sK, long long sV, long long sO,
                       float scale, void* stream);

/* dcp.py:144-154 LayerNorm: out = a*(x-mean)/(std+eps)+b over the last dim D (torch.std: unbiased) [+ residual].
 * D a multiple of 4; x, a, b, residual and out contiguous and 16-byte aligned. */
int houv_layernorm(const float* x, long long rows, int D, const float* a, const float* b, float eps,
                   const float* residual_or_null, float* out, void* stream);

/* dcp.py:31: x[rows,L] <- softmax over L, in place. */
int houv_softmax_rows(float* x, long long rows, int L, void* stream);

/* dcp.py:346-348: corr[P,3,N] = pts[P,M,3]^T . softmax(scores[P,N,M])^T, one pass per score row. */
int houv_softmax_corr(const float* scores, int P, int N, int M, const float* pts, float* corr, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sibling point ops of utils/mm3d_pn2 (call site registration/train_utils.py:459-464 `combine`).
 * The reference's CUDA extensions cannot run here and it holds no fixtures for them: parity unpinned. */

/* furthest_point_sample (utils/mm3d_pn2/ops/furthest_point_sample/furthest_point_sample.py:15-36): idx[B,npoint],
 * starting from point 0, each next sample = the point furthest from the chosen set (lowest index on ties). */
int houv_furthest_point_sample(const float* xyz, int B, int N, int npoint, int32_t* idx, void* stream);

/* three_nn generalised (utils/mm3d_pn2/ops/interpolate/three_nn.py:11-37): the k (1..32, k <= M) nearest points of
 * ref[B,M,3] for every query[B,N,3], nearest first (the lower index first among equal distances): dist2[B,N,k] SQUARED
 * distances, idx[B,N,k].  k = 1, 3, 8 have kernels of their own; any other k runs the next list size up (3, 8, 16, 32) and
 * writes its first k entries, which are the k-list. */
int houv_knn_cross(const float* query, const float* ref, int B, int N, int M, int k, float* dist2, int32_t* idx,
                   void* stream);

/* gather_points (utils/mm3d_pn2/ops/gather_points/gather_points.py:14-35): out[B,C,M] = features[B,C,idx[B,M]]. */
int houv_gather_points(const float* features, const int32_t* idx, int B, int C, int N, int M, float* out, void* stream);

/* ball_query (utils/mm3d_pn2/ops/ball_query/src/ball_query_cuda.cu:11-54).  For every centre center[b,c] the points xyz[b,k],
 * k = 0..N-1 in index order, are tested with d2 = ((cx-x)*(cx-x) + (cy-y)*(cy-y)) + (cz-z)*(cz-z) (fp32, no contraction): a
 * point is a hit iff d2 == 0 || (d2 >= min_radius*min_radius && d2 < max_radius*max_radius), the radii squared in fp32.  The
 * first nsample hits go to idx[b,c,0..] in index order; unused slots repeat the first hit; with no hit every slot is 0 (every
 * slot is written here: the output need not be zero-filled).  cnt_or_null[b,c] = the number of hits, capped at nsample.
 * 1 <= N, 1 <= nsample <= 64, min_radius < max_radius. */
int houv_ball_query(const float* xyz, const float* center, int B, int N, int Mc, float min_radius, float max_radius,
                    int nsample, int32_t* idx, int32_t* cnt_or_null, void* stream);

/* three_interpolate forward (utils/mm3d_pn2/ops/interpolate/src/three_interpolate_cuda.cu): features[B,C,M], idx[B,N,3] in
 * [0,M), weight[B,N,3] -> out[b,c,i] = (w0*f[idx0] + w1*f[idx1]) + w2*f[idx2] with f = features[b,c]. */
int houv_three_interpolate(const float* features, const int32_t* idx, const float* weight, int B, int C, int M, int N,
                           float* out, void* stream);

/* The backward pass of gather_points (S = 1, idx[B,M]), grouping_operation (S = 1, idx[B,npoint*nsample]) and
 * three_interpolate (S = 3, idx and weight viewed as [B,N*3]): grad_out[B,C,M/S], idx[B,M] in [0,N), weight_or_null[B,M] ->
 * grad_features[b,c,k] = the fp32 sum, over m ASCENDING with idx[b,m] == k, of grad_out[b,c,m/S] * weight[b,m] (the product
 * first; no weight: the term is grad_out itself), the additions sequential in that order starting from the first term.
 * Every element of grad_features is written, 0 where nothing lands.  No float atomics: the result is bit-identical from call
 * to call and to the sequential host loop.  An idx outside [0,N) contributes nothing.  `workspace` is caller-allocated device
 * memory of houv_scatter_points_workspace_bytes(B, N, M) bytes (4-byte aligned; contents on entry ignored).  M % S == 0. */
int houv_scatter_points_grad(const float* grad_out, const int32_t* idx, const float* weight_or_null, int B, int C, int N,
                             int M, int S, float* grad_features, void* workspace, void* stream);

/* Bytes of the workspace houv_scatter_points_grad needs (0 for arguments out of range). */
long long houv_scatter_points_workspace_bytes(int B, int N, int M);

/* ---------------------------------------------------------------------------------------------
 * Earth mover's distance by the auction algorithm.
 * Replaces: pybind `emd.forward` / `emd.backward` (utils/metrics/EMD/emd.cpp, emd_cuda.cu; emd_module.py:54-95), with the
 * reference's semantics made exact where its award step races.  xyz1[B,N,3] are the bidders ("the prediction"), xyz2[B,M,3]
 * the objects ("the ground truth"); N == M in 1..16384, any B, eps > 0 (finite), iters >= 1.
 * Per cloud: price[j] = 0, assign[i] = -1, owner[j] = -1; for t = 0 .. iters-1:
 *   U = { i : assign[i] == -1 }; U empty -> stop (exact: later iterations change nothing);
 *   bid: v_ij = (3.0f - sqrtf((dx*dx + dy*dy) + dz*dz)) - price[j], d = xyz2[j] - xyz1[i], fp32, no contraction, sqrtf
 *        correctly rounded; j* = argmax_j v_ij (lowest j on ties); second = max_{j != j*} v_ij (= best when N == 1);
 *        inc_i = (best - second) + eps;
 *   award: each object that received bids goes to the largest inc, ties to the lowest i.  t < iters-1: the previous owner
 *        is evicted (assign = -1), owner[j] = winner, assign[winner] = j, price[j] += inc_winner.  t == iters-1: every
 *        bidder in U takes its bid object, no eviction (complete, not necessarily a bijection, as in the reference).
 * Outputs: dist[B,N] = (dx*dx + dy*dy) + dz*dz with d = xyz1[i] - xyz2[assignment[i]] (SQUARED distance, reference
 * CalcDist); assignment[B,N] int32; iters_run[B] (may be NULL) the iterations each cloud actually ran (< iters: the auction
 * finished before the forced last step).
 * N <= 4096 runs entirely in LDS and takes no workspace; 4097..16384 needs a caller-allocated device workspace of
 * houv_emd_workspace_bytes(B, N) bytes (no alignment beyond 4 bytes; its contents on entry are ignored).  Nothing is allocated
 * in here.  Results are deterministic: bit-identical from call to call and to the sequential restatement of this contract.
 * Non-finite coordinates are the caller's error but stay in range: a bidder whose values are all NaN bids for object 0 with a
 * NaN increment (whose bits outrank every finite key, so it takes object 0 and keeps it), its dist is NaN, every assignment
 * stays in [0, N), and the other clouds of the batch are not affected.
 * Returns 0 with houv_last_error() set, launching nothing, when a check fails. */
int houv_emd_forward(const float* xyz1, const float* xyz2, int B, int N, int M, float eps, int iters, float* dist,
                     int32_t* assignment, int32_t* iters_run_or_null, void* workspace_or_null, void* stream);

/* Bytes of the workspace houv_emd_forward needs for B clouds of N points: 0 for N <= 4096 (and for arguments out of range). */
long long houv_emd_workspace_bytes(int B, int N);

/* Replaces: pybind `emd.backward` (emd_cuda.cu NmDistanceGradKernel).  ACCUMULATES into gradxyz1[B,N,3], which the caller
 * must have zero-filled: gradxyz1[b,i] += (2*graddist[b,i]) * (xyz1[b,i] - xyz2[b,assignment[b,i]]).  The gradient of xyz2
 * is zero, as the reference returns; nothing is written for it.  1 <= N <= 16384. */
int houv_emd_backward(const float* xyz1, const float* xyz2, int B, int N, const float* graddist, const int32_t* assignment,
                      float* gradxyz1, void* stream);

/* ---------------------------------------------------------------------------------------------
 * DeepGMR head (registration/models/deepgmr.py): the two pieces the reference runs on the host.
 * fp32 data, fixed expression trees, no allocation, no atomics; each returns 0 with houv_last_error() set, launching nothing,
 * when a check fails. */

/* get_rri_cluster (deepgmr.py:54-95).  xyz[B,N,3]; idx[B,N,idx_ld] neighbour lists into the SAME cloud, of which entries
 * idx[b,n,idx_skip + j], j = 0..k-1, are used (2 <= k <= 31, idx_skip + k <= idx_ld; an entry outside 0..N-1 is clamped into
 * that range).  out[B,N,4k], channel 4*j + f, every element written.  For point p with neighbours q_j:
 *   f=0  rp = |p| = sqrt((x*x + y*y) + z*z)            f=1  rq_j = |q_j|
 *   f=2  theta_j = acos(clamp(pn.qn_j, -1, 1)),  pn = p/rp, qn_j = q_j/rq_j, dot = (x*x' + y*y') + z*z'
 *        T_j = q_j - (pn.qn_j) * p        (the cosine multiplies the UNNORMALISED p, as the reference does)
 *        psi[j,i] = atan2((T_i x T_j).pn, T_i.T_j); a negative value gets float32(2 pi) added; -0 -> 0
 *   f=3  phi_j = the second smallest of {psi[j,i] : i = 0..k-1} as a multiset, NaNs ranking last (np.sort order); NaN when
 *        fewer than two are not NaN.
 * A zero-norm point yields IEEE results (rp = 0, NaN theta/phi where it takes part); nothing is special-cased. */
int houv_rri_features(const float* xyz, const int32_t* idx, int B, int N, int k, int idx_ld, int idx_skip, float* out,
                      void* stream);

/* gmm_params (deepgmr.py:98-120).  gamma[B,N,J] responsibilities, pts[B,N,3]; 1 <= J <= 32, N >= 1.
 *   pi[B,J]    = (sum_n gamma[n,j]) / N
 *   mu[B,J,3]  = (sum_n gamma[n,j] p_n) / (N pi_j)
 *   sigma[B,J] = (sum_n gamma[n,j] |p_n - mu_j|^2) / (N pi_j)   one scalar: the reference's isotropic sigma*I, NOT divided by 3
 * Two passes (mu first, then the deviations about it); one workgroup per cloud; sums run over a fixed tree, so results are
 * bit-identical from call to call. */
int houv_gmm_params(const float* gamma, const float* pts, int B, int N, int J, float* pi, float* mu, float* sigma,
                    void* stream);

/* gmm_register (deepgmr.py:123-143).  pi_s[B,J], mu_s[B,J,3], mu_t[B,J,3], sigma_t[B,J] (houv_gmm_params' scalar); J >= 1.
 *   c_s = sum_j pi_s,j mu_s,j;  c_t = sum_j pi_s,j mu_t,j   (pi_s weights both, as in the reference)
 *   Ms = sum_j pi_s,j (mu_s,j - c_s)(mu_t,j - c_t)^T / sigma_t,j = U S V^T (singular values sorted, one-sided Jacobi)
 *   R = V diag(1, 1, det(V U^T)) U^T;  t = c_t - R c_s;  T[B,4,4] = [[R, t], [0, 0, 0, 1]]
 * The sums and the SVD run in float64 registers on the fp32 inputs (one lane per pair: the arithmetic is free); T is rounded
 * to fp32 once.  A zero sigma_t propagates inf/NaN into T, as the reference's sigma.inverse() does. */
int houv_gmm_register(const float* pi_s, const float* mu_s, const float* mu_t, const float* sigma_t, int B, int J, float* T,
                      void* stream);

/* ---------------------------------------------------------------------------------------------
 * DeepGMR training: the backward of the two GMM kernels above, and training-mode BatchNorm on
 * point-major rows.  fp32 data, fixed expression trees, no allocation, no float atomics: every sum runs in an order fixed by
 * the shape, so results are bit-identical from call to call.  Each returns 0 with houv_last_error() set, launching nothing,
 * when a check fails. */

/* Backward of (pi, mu, sigma) = houv_gmm_params(gamma = softmax(logits), pts) with the softmax's folded in.  gamma[B,N,J],
 * pts[B,N,3], pi / mu / sigma as houv_gmm_params returned them, g_pi[B,J], g_mu[B,J,3], g_sigma[B,J]; 1 <= J <= 32.
 * With S0_j = N pi_j and d = p_n - mu_j:
 *   gg[n,j]       = g_pi_j / N + ((g_mu_j . d) + g_sigma_j (|d|^2 - sigma_j)) / S0_j
 *   g_logits[n,j] = gamma[n,j] (gg[n,j] - sum_i gamma[n,i] gg[n,i])
 * One pass, one point per group of J lanes; nothing of size [B,N,J,3] is built.  pts gets no gradient. */
int houv_gmm_params_backward(const float* gamma, const float* pts, const float* pi, const float* mu, const float* sigma,
                             const float* g_pi, const float* g_mu, const float* g_sigma, int B, int N, int J, float* g_logits,
                             void* stream);

/* Backward of T = houv_gmm_register(pi_s, mu_s, mu_t, sigma_t): g_T[B,4,4] (its bottom row is ignored) -> g_pi_s[B,J],
 * g_mu_s[B,J,3], g_mu_t[B,J,3], g_sigma_t[B,J].  One lane per pair, float64 registers, the forward recomputed.  The rotation's
 * derivative is taken in polar form, not through the SVD's (whose 1 / (s_i^2 - s_j^2) terms blow up at equal singular values
 * although they cancel): with Ms = U S V^T, R = V D U^T, D = diag(1, 1, det(V U^T)), lam = (s1, s2, D33 s3),
 *   G_R = g_T[:3,:3] - g_t c_s^T,   A~ = U^T skew(R^T G_R) U,   B~_ij = A~_ij / (lam_i + lam_j) (i != j),   skew(X) = (X - X^T)/2
 *   g_Ms = -2 U B~ U^T R^T;   g_c_t = g_t,   g_c_s = -R^T g_t
 * and the chain through Ms, c_s, c_t (pi_s weights both centres) gives the four outputs.  A pair with lam_i + lam_j = 0 (the
 * rotation is then undetermined) yields inf/NaN. */
int houv_gmm_register_backward(const float* pi_s, const float* mu_s, const float* mu_t, const float* sigma_t, const float* g_T,
                               int B, int J, float* g_pi_s, float* g_mu_s, float* g_mu_t, float* g_sigma_t, void* stream);

/* Training-mode BatchNorm over rows z[R,C] with row stride ld >= C (floats); C >= 1.  Rows are handled in chunks of 128: a
 * chunk's column sums are formed by one workgroup in a fixed order, written to the workspace and combined in chunk order by a
 * second launch.  workspace: houv_bn_rows_workspace_bytes(R, C, N_group) bytes (0 for arguments out of range), 16-byte aligned;
 * its contents are scratch.  16-byte loads are used where C, the strides and the pointers are multiples of 4 floats.
 *
 * houv_bn_rows_stats (R >= 2): mean[C] and the biased variance var[C] about it; per chunk (mean, M2) by two passes, chunks
 * merged as (count, mean, M2) -- never E[z^2] - mean^2. */
long long houv_bn_rows_workspace_bytes(long long R, int C, int N_group);
int houv_bn_rows_stats(const float* z, long long R, int C, long long ld, float* mean, float* var, void* workspace,
                       long long workspace_bytes, void* stream);

/* y[R,C] (row stride ldy) = relu?(((z - mean) * rstd) * weight + bias), rstd = 1 / sqrt(var + eps).  With
 * N_group > 0 (it must divide R) also gmax[R/N_group, C] and garg[R/N_group, C]: the column maximum of y over each group of
 * N_group consecutive rows and the lowest row index (0 <= garg < R, counted over all rows) that attains it; NaN never attains
 * a maximum.  The workspace is needed for N_group > 128 only and may be NULL otherwise. */
int houv_bn_relu_rows(const float* z, long long R, int C, long long ld, const float* mean, const float* var, const float* weight,
                      const float* bias, float eps, int relu, int N_group, float* y, long long ldy, float* gmax, int32_t* garg,
                      void* workspace, long long workspace_bytes, void* stream);

/* Backward of houv_bn_relu_rows with mean / var the batch statistics of z: gy[R,C] (row stride ldg) -> gz[R,C] (row stride
 * ldz), gweight[C], gbias[C].  xhat and the ReLU mask are recomputed from z with the forward's expression; g = gy [y > 0];
 *   gbias = sum_r g,  gweight = sum_r g xhat,  gz = (weight rstd) ((g - gbias / R) - xhat (gweight / R)).
 * gz may be gy. */
int houv_bn_relu_rows_backward(const float* gy, long long ldg, const float* z, long long R, int C, long long ld, const float* mean,
                               const float* var, const float* weight, const float* bias, float eps, int relu, float* gz,
                               long long ldz, float* gweight, float* gbias, void* workspace, long long workspace_bytes,
                               void* stream);

/* ---------------------------------------------------------------------------------------------
 * IDAM head (registration/models/idam.py).  fp32 data, fixed expression trees, no allocation, no atomics:
 * results are bit-identical from call to call.  Each returns 0 with houv_last_error() set, launching nothing, when a check
 * fails. */

/* One iteration's similarity stage (idam.py:267-320), fused: nothing of size Ms x Mt reaches memory unless `scores` is given.
 * src[B,Ms,3], tgt[B,Mt,3] points; es[B,Ms,E], et[B,Mt,E] embeddings as rows (16-byte aligned); E a multiple of 4 in 4..128;
 * Ms, Mt >= 1; any B (B = 0 launches nothing).  Layer parameters, eval-mode BatchNorm folded to per-channel scale/shift by the
 * caller: W1[32, 2E+4] (columns: E of es, E of et, distance, unit direction x y z), s1[32], t1[32]; W2[32,32], b2[32];
 * W3[32,32], s3[32], t3[32]; w4[32], b4[1] (a device pointer, like the rest).  Per pair (i, j), all fp32:
 *   diff = src_i - tgt_j;  d = sqrtf((dx*dx + dy*dy) + dz*dz);  u = diff / (d + 1e-8f)        (d = 0 gives u = 0, not NaN)
 *   pre_c = (W1[c,:E].es_i + W1[c,E:2E].et_j) + fma(W1[c,2E+3], uz, fma(W1[c,2E+2], uy, fma(W1[c,2E+1], ux, W1[c,2E]*d)))
 *           the two dot products: sequential fma chains over e ascending, starting from 0
 *   h1_c = max(fma(s1_c, pre_c, t1_c), 0)
 *   h2_c = b2_c + sum_k W2[c,k] h1_k                  (an fma chain over k ascending starting from b2_c)
 *   h3_c = max(fma(s3_c, sum_k W3[c,k] h2_k, t3_c), 0)   (chain from 0)
 *   score = clamp(b4 + sum_c w4_c h3_c, -20, 20)          (chain over c ascending starting from b4)
 * Outputs, each may be NULL:
 *   rowmax[B,Ms,32]   max over j of h2 (the reference takes it before sim_mat_conv2, :289)
 *   corr_idx[B,Ms]    arg-max over j of score, the LOWEST j among equal scores (rows clamped at +-20 make that a real case)
 *   corr[B,3,Ms]      tgt[corr_idx], channel-major: houv_kabsch's operand
 *   scores[B,Ms,Mt]   the clamped scores */
int houv_idam_simmat(const float* src, const float* tgt, const float* es, const float* et, int B, int Ms, int Mt, int E,
                     const float* W1, const float* s1, const float* t1, const float* W2, const float* b2, const float* W3,
                     const float* s3, const float* t3, const float* w4, const float* b4, float* rowmax_or_null,
                     int32_t* corr_idx_or_null, float* corr_or_null, float* scores_or_null, void* stream);

/* Propagate's edge features (idam.py:121-124): X[B,N,C] rows, idx[B,N,idx_ld] neighbour lists into the SAME cloud, of which the
 * first k entries of a row are used (k <= idx_ld; an entry outside 0..N-1 is clamped into that range).
 *   out[((b*N + n)*k + j)*ldo + c] = X[b, idx[b,n,j], c] - X[b,n,c]   for c < C;   0 for C <= c < ldo   (ldo >= C)
 * Every element of out[B*N*k, ldo] is written.  No alignment is required; 16-byte moves are used when C and ldo are multiples
 * of 4 and X and out are 16-byte aligned. */
int houv_edge_diff(const float* X, const int32_t* idx, int B, int N, int k, int C, int idx_ld, int ldo, float* out,
                   void* stream);

/* ---------------------------------------------------------------------------------------------
 * PCN completion network (registration/models/pcn.py).  fp32 in, fp32 out, products on the fp32-input
 * MFMA (an ordered fma chain over k); no allocation, no atomics, fixed reduction orders: results are bit-identical from call to
 * call.  Activations are rows [points, channels], weights [out, in] row-major, all densely packed; no pointer needs more than
 * its natural 4-byte alignment.  Each returns 0 with houv_last_error() set, launching nothing, when a check fails. */

/* Points per workgroup of both kernels: the row tile at whose edges a partial tile begins. */
#define HOUV_PCN_ROW_TILE 64

/* One PointNet block: a two-layer pointwise MLP with the channel-wise maximum over each cloud's points as its epilogue.
 *   y[b,n,c]    = W2[c,:] . relu(W1 . x[b,n,:] + shift1[b,:]) + b2[c]
 *   pooled[b,c] = max over n < N of y[b,n,c]            (a true maximum: all-negative columns pool to a negative value)
 *                 A NaN in y is stored in y but does NOT reach pooled: the maximum skips NaN (fmaxf), where torch.max
 *                 propagates it; a column that is NaN in every row pools to -inf.
 * x[B,N,Cin], W1[H,Cin], W2[Cout,H], b2[Cout]; shift1 is read at shift1 + b * shift1_stride (floats): stride 0 is one bias
 * shared by all clouds, otherwise stride >= H.  Served (Cin, H, Cout): (3, 128, 256) and (256, 512, 1024); N >= 1; any B (B = 0
 * launches nothing).  pooled[B,Cout] is always written; y_or_null[B,N,Cout] receives the pre-pool activations when given.  The
 * hidden [B,N,H] activations never reach memory.  When N spans more than one row tile the per-tile maxima pass through
 * `workspace` (houv_mlp2_max_workspace_bytes(B, N, Cout) bytes, caller-allocated; may be NULL when that is 0). */
int houv_mlp2_max(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1, long long shift1_stride,
                  const float* W2, const float* b2, int Cout, float* pooled, float* y_or_null, float* workspace, void* stream);
long long houv_mlp2_max_workspace_bytes(int B, int N, int Cout);

/* houv_mlp2_max that also reports where each maximum was found: the arguments, checks and served
 * shapes of houv_mlp2_max plus arg[B,Cout].  pooled and y are bit-identical to houv_mlp2_max's.
 *   arg[b,c] = the LOWEST n with y[b,n,c] == pooled[b,c]   (float equality; the rule of torch.max(x, 2) on the CPU, where a
 *              tied maximum returns its first index and receives the whole gradient)
 * A column that is NaN in every row has no such n: arg = -1 (its pooled is -inf, as above), and a backward pass sends no
 * gradient through it.  A column whose largest value is a true -inf reports the first row holding it.  The per-tile
 * (maximum, row) pairs pass through `workspace` (houv_mlp2_max_arg_workspace_bytes(B, N, Cout) bytes, twice the plain call's;
 * may be NULL when that is 0); the first tile that attains the maximum keeps it. */
int houv_mlp2_max_arg(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
                      long long shift1_stride, const float* W2, const float* b2, int Cout, float* pooled, int32_t* arg,
                      float* y_or_null, float* workspace, void* stream);
long long houv_mlp2_max_arg_workspace_bytes(int B, int N, int Cout);

/* The backward pass of one PointNet block, evaluated on the ACTIVE rows only.  With
 *   h = relu(W1 x + shift1[b]),  z = W2 h + b2,  pooled = max over n of z   (houv_mlp2_max_arg gave arg)
 * the gradient of pooled[b,c] reaches row arg[b,c] alone (arg < 0 or >= N: no row, no gradient).  A gradient on y itself may
 * come along on a list of rows per cloud: rows[B,R] (STRICTLY ascending in each cloud's first nrows[b] <= R entries, the
 * rest ignored), gy_rows[B,R,Cout] (the gradient of y[b, rows[b,k], :]); R = 0 with NULL for the three: no such gradient.
 * Let A_b = set(arg[b,:]) u rows[b]; it has at most Rcap = houv_mlp2_max_backward_rows(N, Cout, R) = min(N, Cout + R) rows.
 *   gz[b,r,c] = gy[b,r,c] + gpooled[b,c] * [arg[b,c] == r]            for r in A_b (never stored)
 *   gb2[Cout] = sum gz;   gW2[Cout,H] = sum gz^T h;   gh = (gz W2) * [h > 0];   gW1[H,Cin] = sum gh^T x
 *   gshift1[B,H] = sum over r in A_b of gh   (always one row per cloud: the caller sums it when shift1 was shared)
 *   gx = gh W1
 * Row-carried outputs are COMPACTED per cloud: act_rows[B,Rcap] holds A_b ascending and -1 in the slots past nact[b] =
 * |A_b|; gx_rows_or_null[B,Rcap,Cin] holds gx of row act_rows[b,p] in slot p and exact zeros in the slots past nact[b].
 * (act_rows, nact, gx_rows) of the block that consumed y is therefore (rows, nrows, gy_rows) of the block that made it.
 * h is recomputed on the active rows by houv_gemm_f32, whose rounding may differ from the forward's in the last place: a
 * hidden unit within that of zero may be masked differently.  Sums run clouds ascending, rows ascending; no atomics; two
 * calls give the same bits.  x, W1, shift1 (+ stride), W2 as in houv_mlp2_max, same served shapes; R >= 0; B <= 65535
 * (B = 0 writes zero weight gradients).  workspace: houv_mlp2_max_backward_workspace_bytes(B, N, Cin, H, Cout, R) bytes,
 * 16-byte aligned, caller-allocated. */
int houv_mlp2_max_backward(const float* x, int B, int N, int Cin, const float* W1, int H, const float* shift1,
                           long long shift1_stride, const float* W2, int Cout, const int32_t* arg, const float* gpooled,
                           const int32_t* rows_or_null, const int32_t* nrows_or_null, const float* gy_rows_or_null, int R,
                           float* gW1, float* gshift1, float* gW2, float* gb2, int32_t* act_rows, int32_t* nact,
                           float* gx_rows_or_null, void* workspace, void* stream);
long long houv_mlp2_max_backward_workspace_bytes(int B, int N, int Cin, int H, int Cout, int R);
int houv_mlp2_max_backward_rows(int N, int Cout, int R);

/* The folding stage of PCN_decoder.forward (pcn.py:108-125).  coarse[B,nc,3], cvec[B,512] (the global feature's share of the
 * first convolution plus its bias, one vector per cloud), grid[2,scale], Wgp[512,5] (the first convolution's columns for the
 * two grid and three centre channels), W2[512,512], b2[512], W3[3,512], b3[3]; nc, scale >= 1.  For fine point f = c*scale + s:
 *   h1 = relu(fma(Wgp[:,4], cz, fma(Wgp[:,3], cy, fma(Wgp[:,2], cx, fma(Wgp[:,1], grid[1,s], Wgp[:,0]*grid[0,s])))) + cvec[b,:])
 *   h2 = relu(W2 . h1 + b2)
 *   fine[b,f,:] = (W3 . h2 + b3) + coarse[b,c,:]
 * fine[B, nc*scale, 3] is the only tensor written. */
int houv_pcn_fold(const float* coarse, const float* cvec, const float* grid, int B, int nc, int scale, const float* Wgp,
                  const float* W2, const float* b2, const float* W3, const float* b3, float* fine, void* stream);

/* The backward pass of houv_pcn_fold: its inputs plus gfine[B, nc*scale, 3], the gradient of fine.
 *   gh2 = (W3^T gfine) * [h2 > 0];  gh1 = (gh2 W2) * [h1 > 0]   per fine point, h1 and h2 recomputed as the forward computes them
 *   gW3[3,512] = sum gfine^T h2;  gb3[3] = sum gfine;  gW2[512,512] = sum gh2^T h1;  gb2[512] = sum gh2
 *   gWgp[512,5] = sum gh1^T (grid[0,s], grid[1,s], coarse[b,c,:]);  gcvec[B,512] = sum over the cloud's fine points of gh1
 *   gcoarse[B,nc,3] = sum over the scale cells s ascending of (gfine[b, c*scale+s, :] + gh1 Wgp[:, 2:5]): the centre path and
 *                     the path through the first convolution
 * (b3 is checked but not read.)  The forward saved nothing.  Row sums leave the kernel as per-tile partials that are added in
 * tile order, gW2 is a houv_gemm_f32 over row chunks whose partials are added in chunk order: no atomics, two calls give the
 * same bits.  workspace: houv_pcn_fold_backward_workspace_bytes(B, nc, scale) bytes, 16-byte aligned, caller-allocated (h1 and
 * the k-major gh2 of every fine point, the partials); `workspace_bytes` is what the caller allocated, and a smaller or NULL
 * workspace is refused.  B = 0 writes zero weight gradients. */
int houv_pcn_fold_backward(const float* coarse, const float* cvec, const float* grid, int B, int nc, int scale, const float* Wgp,
                           const float* W2, const float* b2, const float* W3, const float* b3, const float* gfine,
                           float* gcoarse, float* gcvec, float* gWgp, float* gW2, float* gb2, float* gW3, float* gb3,
                           void* workspace, long long workspace_bytes, void* stream);
long long houv_pcn_fold_backward_workspace_bytes(int B, int nc, int scale);

/* ---------------------------------------------------------------------------------------------
 * ECG completion network (completion/models/ecg.py).  fp32 data, fixed expression trees, no allocation,
 * no atomics, no scratch: results are bit-identical from call to call.  Each returns 0 with houv_last_error() set, launching
 * nothing, when a check fails (a NULL pointer included). */

/* Candidates per register block and channels per chunk of houv_knn_feat: the sizes at whose edges a partial block begins. */
#define HOUV_KNN_FEAT_BLOCK 32
#define HOUV_KNN_FEAT_CHUNK 16
/* Growth rate of houv_dense_conv (the G of ecg.py's Dense_conv as ECG builds it). */
#define HOUV_DENSE_CONV_GROWTH 24

/* k nearest neighbours in feature space (get_graph_feature's knn, completion/model_utils.py).  x[B,N,C] token-major rows of
 * stride ldx >= C floats; idx[B,N,k] and dist2_or_null[B,N,k] nearest first; the point itself is a candidate.
 * 1 <= C <= 256, 1 <= k <= 32, k <= N <= 16384, B <= 65535 (B = 0 launches nothing).
 * The ranked value is, in fp32:   d = 0;  for c = 0 .. C-1:  t = x[j,c] - x[i,c];  d = fmaf(t, t, d)
 * and equal d puts the lower index first (the stable insertion of houv_knn_cross).  With C = 3 this is houv_knn_cross(x, x)'s
 * value bit for bit.  The chain is order-defined, so a host function reproduces idx AND dist2 exactly.
 * The reference ranks the expanded form -|a|^2 + 2ab - |b|^2 in fp32 with torch.topk, which cancels where two rows are close:
 * it differs from this (and from itself in float64) at near-ties, 17-112 of the 16384 entries of a 1024 x 16 list measured on
 * its own activations.  The [B,N,N] matrix it builds does not exist here. */
int houv_knn_feat(const float* x, int B, int N, int C, int ldx, int k, int32_t* idx, float* dist2_or_null, void* stream);

/* Dense_conv.forward (ecg.py:58-65) with growth rate G = 24 and dense_n = 3, fused through the maximum over the neighbours.
 * x[B,N,C] rows of stride ldx >= C; idx[B,N,k] neighbour lists into the SAME cloud (an entry outside 0..N-1 is clamped into
 * that range: nothing outside x is read); W0[G,2C], W1[G,G+C], W2[G,2G+C] row-major, b0, b1, b2[G].  For point i, neighbour j:
 *   e  = cat(x_i, x_j - x_i)                      y0 = relu(W0 e + b0)
 *   s1 = relu(W1 cat(y0, x_i) + b1)               s2 = W2 cat(y0, x_i, s1) + b2          (no activation)
 *   out[b,i,:] = max over the k neighbours of cat(y0, x_i, s1, s2)       channel order G, C, G, G as the reference has it
 * The maximum starts from -inf (s2 may be negative for every neighbour) and skips NaN (fmaxf), where torch.max propagates it: a
 * column that is NaN for every neighbour pools to -inf.  relu_out != 0 applies max(., 0) to the result (the caller's F.relu).
 * out rows have stride ldo >= C + 3G; columns C + 3G .. ldo-1 are not touched, so the caller can point `out` into a wider
 * buffer.  Products are fma chains in the reference's column order; the x_i columns of the three layers are evaluated once per
 * point (W0's lead its chain, W1's and W2's are added to the per-edge part).  Served: C = 24 and C = 48, 1 <= k <= 32, N >= 1,
 * B <= 65535; anything else is refused by name.  No [B, ., N, k] tensor exists anywhere. */
int houv_dense_conv(const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k, const float* W0, const float* b0,
                    const float* W1, const float* b1, const float* W2, const float* b2, int relu_out, float* out, int ldo,
                    void* stream);

/* houv_dense_conv that also reports where each maximum was found: the arguments, checks and served
 * shapes of houv_dense_conv plus arg[B,N,72] (int8, 4-byte aligned; the pooled columns in the order y0 (24), s1 (24), s2 (24)).
 * `out` is written by houv_dense_conv's own kernels and is bit-identical to its result.  A second pass, a kernel of its own,
 * recomputes the three layers by the same chains and keeps
 *   arg[b,i,q] = the LOWEST edge slot e in 0 .. k-1 whose candidate attains the maximum of pooled column q   (torch.max's rule
 *                on the CPU: a tied maximum returns its first index and receives the whole gradient)
 * A column that is NaN for every neighbour has no such e: arg = -1 (it pools to -inf, as above), and a backward pass sends no
 * gradient through it.  A column whose largest candidate is a true -inf reports the first slot holding it. */
int houv_dense_conv_arg(const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k, const float* W0, const float* b0,
                        const float* W1, const float* b1, const float* W2, const float* b2, int relu_out, float* out, int ldo,
                        int8_t* arg, void* stream);

/* The backward pass of houv_dense_conv: its inputs, arg from houv_dense_conv_arg, the forward's out
 * (rows of stride ldo; read only when relu_out is set, NULL allowed otherwise) and gout[B,N,C+72] (rows of stride ldg >= C + 72),
 * the gradient of out.  With g = gout * [out > 0] when relu_out is set and g = gout otherwise, point i, edge slot e,
 * j = clamp(idx[i,e], 0, N-1), y0 and s1 recomputed by the forward's own fma chains (the ReLU masks are the forward's bits):
 *   gs2[o] = g[2G+C+o] * [arg[2G+o] == e]
 *   gs1[c] = ((sum_o W2[o,G+C+c] gs2[o]) + g[G+C+c] * [arg[G+c] == e]) * [s1[c] > 0]
 *   gy0[c] = (((sum_o W1[o,c] gs1[o]) + (sum_o W2[o,c] gs2[o])) + g[c] * [arg[c] == e]) * [y0[c] > 0]      sums o ascending, fma
 * and per point Gy0 = sum_e gy0 (e ascending), Gs1 = sum_e gs1, Gs2[o] = g[2G+C+o] * [arg[2G+o] >= 0],
 * D[m] = the sum of gy0 over the edges (i, e) with j == m in ascending (i, e) order (the neighbour path lands on the CLAMPED row):
 *   gx[b,i,c] = (((P1 + P2) + P3) + P4) + g[G+c]   (the pass-through columns last), each P an fma chain from 0, o ascending:
 *               P1 = sum_o W1[o,G+c] Gs1[o],  P2 = sum_o W2[o,G+c] Gs2[o],  P3 = sum_o W0[o,c] Gy0[o],
 *               P4 = sum_o W0[o,C+c] (D[i][o] - Gy0[o])
 *   gW0[G,2C] = sum (Gy0 (x) x_i | gy0 (x) (x_j - x_i));   gW1[G,G+C] = sum (gs1 (x) y0 | Gs1 (x) x_i)
 *   gW2[G,2G+C] = sum (gs2 (x) y0 | Gs2 (x) x_i | gs2 (x) s1);   gb0, gb1, gb2[G] = sum Gy0, Gs1, Gs2
 * Every output is written, not accumulated: gx rows have stride ldgx >= C (columns C .. ldgx-1 are not touched).  Weight
 * gradients are reduced inside each workgroup of 128 points (edges ascending, points ascending), leave as one row of partials
 * per workgroup and are added in workgroup order; D is houv_scatter_points_grad's ordered sum.  No float atomics: two calls give
 * the same bits.  The only tensor with a [B,N,k,.] shape is gy0[B,24,N*k] in the workspace.  Served shapes and refusals are
 * houv_dense_conv's (N * k < 2^31 besides); B = 0 writes zero weight gradients.  workspace:
 * houv_dense_conv_backward_workspace_bytes(B, N, C, k) bytes (0 for arguments out of range), 16-byte aligned, caller-allocated;
 * `workspace_bytes` is what the caller allocated, and a smaller or NULL workspace is refused. */
int houv_dense_conv_backward(const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k, const float* W0,
                             const float* b0, const float* W1, const float* b1, const float* W2, const float* b2, int relu_out,
                             const int8_t* arg, const float* out_or_null, int ldo, const float* gout, int ldg, float* gx, int ldgx,
                             float* gW0, float* gb0, float* gW1, float* gb1, float* gW2, float* gb2, void* workspace,
                             long long workspace_bytes, void* stream);
long long houv_dense_conv_backward_workspace_bytes(int B, int N, int C, int k);

/* ---------------------------------------------------------------------------------------------
 * VRCNet completion network (completion/models/vrcnet.py).  The same promises as the ECG block above. */

/* Points per workgroup of houv_sa_attn: the size at whose edges a partial workgroup begins. */
#define HOUV_SA_ATTN_BLOCK 128

/* SA_module.forward (vrcnet.py:49-67) after its three input projections.  With rel = C/16, mid = C/4, m = mid/8 (share_planes =
 * 8), the caller first writes, with one GEMM per point, P[B,N,2 rel + mid] = relu(x) . [W1; W2; W3]^T + [b1; b2; b3], columns
 * [x1 | x2 | x3], rows of stride ldp.  idx[B,N,k] are neighbour lists into the SAME cloud (an entry outside 0..N-1 is clamped into
 * that range: nothing outside P is read).  For point n:
 *   t[0 .. rel)        = x1[n]
 *   t[rel + r k + j]   = x2[idx[n,j]][r]                     channel-major, neighbour-minor: the reference's x2.view(B,-1,1,N)
 *   h    = relu(Ww1 relu(t))                                 Ww1[m, rel (k+1)] row-major, no bias
 *   w    = Ww2 h + bw2                                       Ww2[k m, m], bw2[k m];  w[c', j] = w[c' k + j]
 *   o[c] = sum over j of w[c mod m, j] x3[idx[n,j]][c]       c in [0, mid): repeat(1, share, 1, 1) tiles the m rows
 *   out[n] = (Wout relu(o) + bout) + x[n]                    Wout[C, mid], bout[C]; x is the PRE-activation identity
 * and relu_out != 0 applies max(., 0) to the result (SK_SA_module's activation).  Every product is an fp32 fma chain in the
 * order written (t: x1 first, then neighbour by neighbour, r ascending; j, q ascending elsewhere).  fmaxf drops a NaN where
 * torch.relu keeps it.
 * x rows have stride ldx >= C, out rows ldo >= C: both may be column slices of wider buffers, and columns C .. ldo-1 of out are
 * not touched.  ldp >= 2 rel + mid must be a multiple of 4 and P aligned to 16 bytes (its rows are read four floats at a time).
 * `out` may be `x` itself (the same pointer and ldo == ldx): an element of x is read only by the lane that then writes it.  The
 * same pointer with ldo != ldx is refused; any other overlap of out with x or P is the caller's error and is not detected.
 * Served: C = 64, 128, 256, 512; 1 <= k <= 32; k <= N <= 16384; B <= 65535 (B = 0 launches nothing); anything else, and a NULL
 * pointer, is refused by name.  No [B, ., k, N] tensor exists anywhere. */
int houv_sa_attn(const float* P, int ldp, const float* x, int ldx, const int32_t* idx, int B, int N, int C, int k,
                 const float* Ww1, const float* Ww2, const float* bw2, const float* Wout, const float* bout, int relu_out,
                 float* out, int ldo, void* stream);

/* The backward pass of houv_sa_attn up to conv_out.  conv_out is two products over all points and stays
 * with the caller on the matrix pipe: with gy = gout * [out > 0] when relu_out was set and gy = gout otherwise, the caller forms
 * G[B,N,mid] = gy . Wout (the gradient of relu(o); rows of stride ldg >= mid), gWout = gy^T . ro and gbout = sum gy; the
 * residual's share of gx is gy itself.  This call takes P, idx, Ww1, Ww2, bw2 as houv_sa_attn does (the same checks, clamping
 * and alignment), recomputes t, pre, h, w and o by the forward's own fma chains (every ReLU mask is the forward's bits), writes
 * ro[B,N,mid] = relu(o) (rows of stride ldro >= mid) and, for point i with n_j = clamp(idx[i,j], 0, N-1):
 *   go[c]      = G[c] * [o[c] > 0]
 *   gw[c',j]   = sum over c = c' (mod m), ascending, of go[c] x3[n_j][c]                      an fma chain from 0
 *   gh[q]      = sum over j, then c', of Ww2[c' k + j, q] gw[c',j];    gpre = gh * [pre > 0]
 *   gt[s]      = [t[s] > 0] * sum over q of Ww1[q,s] gpre[q]
 *   gbw2[c' k + j] = sum_i gw[c',j];   gWw2[c' k + j, q] = sum_i gw[c',j] h[q];   gWw1[q,s] = sum_i gpre[q] relu(t[s])
 *   gP[i, r]           = gt_i[r]                                                               the point's own x1 columns
 *   gP[n, rel + r]     = sum over the edges (i,j) with n_j == n of gt_i[rel + r k + j]
 *   gP[n, 2 rel + c]   = sum over the same edges of go_i[c] w_i[c mod m, j]                    an fma chain from 0
 * The edge sums run in ascending (i, j); a clamped index sends its gradient to the clamped row.  The weight gradients are sums
 * over fixed chunks of consecutive points (ascending inside a chunk), added in chunk order.  No float atomics: two calls give the
 * same bits.  Every output is written, not accumulated; gP rows have stride ldgp >= 2 rel + mid and columns beyond are not
 * touched.  Every float buffer of the workspace is per point ([B,N,w] with w <= rel (k+1) + k m + 2 mid); the only arrays with
 * N k entries per cloud are int32 (the keys and the CSR inverse of idx).  Served shapes and refusals are houv_sa_attn's (N * k <
 * 2^31 besides); B = 0 writes zero weight gradients.  workspace: houv_sa_attn_backward_workspace_bytes(B, N, C, k) bytes (0 for
 * arguments out of range), 16-byte aligned, caller-allocated; `workspace_bytes` is what the caller allocated, and a smaller or
 * NULL workspace is refused. */
int houv_sa_attn_backward(const float* P, int ldp, const int32_t* idx, int B, int N, int C, int k, const float* Ww1,
                          const float* Ww2, const float* bw2, const float* G, int ldg, float* gP, int ldgp, float* ro, int ldro,
                          float* gWw1, float* gWw2, float* gbw2, void* workspace, long long workspace_bytes, void* stream);
long long houv_sa_attn_backward_workspace_bytes(int B, int N, int C, int k);

/* edge_preserve_sampling's feature half (model_utils.py:90-116) as one gather: feat[B,N,C] rows of stride
 * ldx >= C, p_idx[B,S] the sampled rows, pn_idx[B,S,pk] each sample's neighbour list (an entry of either outside 0..N-1 is clamped
 * into that range: nothing outside feat is read) ->
 *   out[b,s,c]     = feat[b, p_idx[b,s], c]
 *   out[b,s,C + c] = max over j of feat[b, pn_idx[b,s,j], c]          c in [0, C); out rows of stride ldo >= 2 C
 * Columns 2 C .. ldo-1 of out are not touched, so `out` may point into a wider buffer.  The maximum keeps a running best that
 * starts at slot 0 and is replaced only by a strictly greater element, so the stored value carries the bits of the winning slot's
 * element and -0 against +0 keeps the earlier slot.  A NaN element is skipped; a column whose pk elements are all NaN is written
 * as NaN.  arg_or_null, when given, is int8 [B,S,C] (dense): the LOWEST slot j that attains the maximum, -1 for an all-NaN column
 * (houv_dense_conv_arg's rule).  The [B,S,pk,C] gather is never built; nothing is allocated; no atomics.  Rows are read and
 * written four floats at a time when C, ldx and ldo are multiples of 4, feat and out aligned to 16 bytes and arg to 4; any other
 * layout runs the same arithmetic one float at a time.  Served: 1 <= C <= 1024, 1 <= pk <= 32, S >= 1 with S (pk + 1) < 2^31,
 * 1 <= N <= 16384, B >= 0 (B = 0 launches nothing); anything else, and a NULL pointer other than arg, is refused by name. */
int houv_edge_pool(const float* feat, int ldx, const int32_t* p_idx, const int32_t* pn_idx, int B, int N, int S, int C, int pk,
                   float* out, int ldo, int8_t* arg_or_null, void* stream);

/* The backward pass of houv_edge_pool: g[B,S,2C] (rows of stride ldg >= 2 C), the forward's lists and arg ->  gfeat[B,N,C] (rows of
 * stride ldgx >= C; columns beyond are not touched), every element written.  gfeat[b,n,c] is the fp32 sum of these terms, added
 * one after the other starting from the first: s ascending; for each s first g[b,s,c] when clamp(p_idx[b,s]) == n, then, j
 * ascending, g[b,s,C+c] when clamp(pn_idx[b,s,j]) == n and arg[b,s,c] == j; +0 where nothing lands.  No float atomics: two calls
 * give the same bits, those of the sequential host loop.  The workspace holds int32 arrays only: the keys [B,S,pk+1] (slot 0 the
 * centre), and their CSR inverse from houv_scatter_points_grad's stable counting sort, offsets [B,N+1] and order [B,S,pk+1].
 * Served shapes, refusals and the vector / scalar layouts are houv_edge_pool's (g, gfeat, arg in place of feat, out, arg).
 * workspace: houv_edge_pool_backward_workspace_bytes(B, N, S, pk) bytes (0 for arguments out of range), 16-byte aligned,
 * caller-allocated; `workspace_bytes` is what the caller allocated, and a smaller, NULL or misaligned workspace is refused. */
int houv_edge_pool_backward(const float* g, int ldg, const int32_t* p_idx, const int32_t* pn_idx, const int8_t* arg, int B, int N,
                            int S, int C, int pk, float* gfeat, int ldgx, void* workspace, long long workspace_bytes, void* stream);
long long houv_edge_pool_backward_workspace_bytes(int B, int N, int S, int pk);

/* EF_expansion (completion/model_utils.py:24-55) past its per-point projections.  proj[B*N, 2 O + 2 O r]
 * = [U | V | P | Q] (rows of stride ldp), idx[B,N,k] (an entry outside 0..N-1 is clamped into that range), W2a[O r, O] (rows of
 * stride ldw: the first O columns of conv2's weight), W3[O,O] and b3[O] (dense).  With m = idx[b,n,j], per sub-row s < r:
 *   h1 = U_n + V_m;   t = W2a[s O : (s+1) O, :] relu(h1) + P_n[s O : (s+1) O] + Q_m[s O : (s+1) O];   e_j = W3 relu(t) + b3
 *   out[b, n r + s, c] = max over j of e_j[c]                           out rows of stride ldo >= O, other columns not touched
 * relu keeps a NaN.  The maximum is houv_edge_pool's: a running best from slot 0 replaced only by a strictly greater value, a NaN
 * skipped, an all-NaN column written as NaN; arg_or_null, when given, is int8 [B, N r, O] (dense), the LOWEST slot that attains
 * the maximum, -1 for an all-NaN column.  Both products run on the fp32-input MFMA.  Nothing is allocated; no atomics.  Served:
 * O in {64, 128, 256}, 1 <= r <= 8, 1 <= k <= 8, 1 <= N <= 16384 with N r O < 2^31, B >= 0 (B = 0 launches nothing); anything
 * else, and a NULL pointer other than arg, is refused by name. */
int houv_ef_expand(const float* proj, int ldp, const int32_t* idx, int B, int N, int O, int k, int r, const float* W2a, int ldw,
                   const float* W3, const float* b3, float* out, int ldo, int8_t* arg_or_null, void* stream);

/* The backward pass of houv_ef_expand: its inputs, the forward's arg and g[B, N r, O] (rows of stride ldg) -> gproj[B*N, 2 O + 2 O r]
 * (rows of stride ldgp, every element of those columns written), gW2a[O r, O], gW3[O, O], gb3[O] (dense).  The forward is
 * recomputed from proj; with ge_j[s][c] = g[b, n r + s, c] where arg == j and +0 elsewhere:
 *   gh2 = W3^T ge (per s);  gt = gh2 [t > 0];  gh1 = (sum over s of W2a_s^T gt_s) [h1 > 0]
 *   gU_n = sum_j gh1;  gP_n = sum_j gt;  gV_m, gQ_m = the same terms over the edges that list m, in ascending (n, j)
 *   gW3 = sum ge (x) relu(t);  gW2a = sum gt (x) relu(h1);  gb3 = sum ge
 * The clouds are taken in groups of whole clouds (about 32768 edges each), one after the other, so the workspace does not grow
 * with B.  A group's per-edge terms go to the workspace; the list sums follow houv_scatter_points_grad's CSR inverse, the weight
 * sums are houv_gemm_f32 products over fixed row chunks whose partials are added to the running sum in chunk order, groups
 * ascending, gb3 per-chunk partials likewise.  No float atomics: two calls give the same bits.  Served shapes and refusals are
 * houv_ef_expand's; B = 0 writes zero weight gradients.  workspace: houv_ef_expand_backward_workspace_bytes(B, N, O, k, r) bytes (0 for arguments out of
 * range), 16-byte aligned, caller-allocated; a smaller, NULL or misaligned workspace is refused. */
int houv_ef_expand_backward(const float* proj, int ldp, const int32_t* idx, const int8_t* arg, int B, int N, int O, int k, int r,
                            const float* W2a, int ldw, const float* W3, const float* g, int ldg, float* gproj, int ldgp,
                            float* gW2a, float* gW3, float* gb3, void* workspace, long long workspace_bytes, void* stream);
long long houv_ef_expand_backward_workspace_bytes(int B, int N, int O, int k, int r);

/* The gradient of the completion Chamfer loss calc_cd(output, gt) with respect to the output cloud.
 * gt[B,N,3], output[B,M,3] and what houv_chamfer_forward(gt, output) gave: dist1[B,N], dist2[B,M], idx1[B,N] (rows of output),
 * idx2[B,M] (rows of gt).  With the upstream gradients g_p[B] of cd_p = (mean sqrt(dist1) + mean sqrt(dist2)) / 2 and g_t[B] of
 * cd_t = mean dist1 + mean dist2:
 *   w1[i] = g_t / N + (g_p / (4 N)) / sqrt(dist1[i]),      w2[j] = g_t / M + (g_p / (4 M)) / sqrt(dist2[j])
 *   gout[b,j] = 2 w2[j] (out[j] - gt[idx2[j]]), then + 2 w1[i] (out[j] - gt[i]) for every i with idx1[i] == j, i ascending
 * gout[B,M,3] is WRITTEN, every element: it need not be zeroed.  No float atomics: a list of up to 32 entries is added one entry
 * after the other; a longer one by 64 lanes (lane l takes entries l, l + 64, ... in order) and a fixed xor butterfly, so the
 * order of every sum is a function of its list and two calls give the same bits, at any B.  A zero distance is not clamped:
 * such a row is NaN, as the composition sqrt -> mean -> backward makes it.  An idx1 entry outside 0..M-1 or an idx2 entry outside
 * 0..N-1 is clamped into that range: nothing outside the clouds is read.  The gradient with respect to gt is not computed.
 * The workspace holds int32 arrays only: the CSR inverse of idx1 from houv_scatter_points_grad's stable counting sort, offsets
 * [B,M+1] and order [B,N]; houv_cd_loss_backward_workspace_bytes(B, N, M) bytes (0 for arguments out of range), 16-byte aligned,
 * caller-allocated; a smaller, NULL or misaligned workspace is refused.  Refused by name: N <= 0, M <= 0, B < 0, a NULL pointer;
 * B = 0 launches nothing. */
int houv_cd_loss_backward(const float* output, const float* gt, const float* dist1, const float* dist2, const int32_t* idx1,
                          const int32_t* idx2, const float* g_p, const float* g_t, int B, int N, int M, float* gout,
                          void* workspace, long long workspace_bytes, void* stream);
long long houv_cd_loss_backward_workspace_bytes(int B, int N, int M);

/* Pose only (HOUV.forward, houv.py:94-103): params fp32 [n,8] -> R[n,9], T[n,3]; if src != NULL
 * also moved[n,N,3] = src[n,N,3] @ R^T + T. */
int houv_pose_forward(const float* params, int n, int angle_base, int trans_mode,
                      const float* src_or_null, int N, float* R, float* T, float* moved_or_null, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HOUV_HIP_H_ */
