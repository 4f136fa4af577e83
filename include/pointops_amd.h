/*
 * pointops_amd.h -- C ABI of libpointops_amd.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary for the batched point-cloud neighbour hot path of
 * pytorch3d_pointops.  Each entry point replaces one operator of the reference's
 * pybind11 module `pytorch3d_pointops._C` (reference: csrc/ext.cpp:15-27); the
 * argument meaning, padding conventions and output layout are the reference's.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc'ed / torch CUDA-HIP tensor storage),
 *     dense row-major, fp32 for point data and int64 for lengths / indices;
 *   - inputs are borrowed and never written; outputs are FULLY written by the call
 *     (padding included), so callers may pass uninitialised buffers;
 *   - `stream` is a hipStream_t (NULL = default stream); calls enqueue work and
 *     return without synchronising (the reference does the same on its current
 *     stream: csrc/knn/knn.cu:331);
 *   - the calling thread's current HIP device must own the buffers;
 *   - return value: 0 on success, a negative POINTOPS_E* code otherwise;
 *     pointops_last_error() gives a thread-local message.
 *   - no torch types, no C++ types, no global state besides the error string.
 */
#ifndef POINTOPS_AMD_H_
#define POINTOPS_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POINTOPS_OK 0
#define POINTOPS_EINVAL (-1)      /* bad argument (shape, norm, K ...)           */
#define POINTOPS_ELAUNCH (-2)     /* HIP launch / runtime error                  */
#define POINTOPS_EWORKSPACE (-3)  /* workspace too small                         */

#define POINTOPS_ABI_VERSION 1

/* Library identification: ABI version and the ISA the kernels were built for. */
int pointops_abi_version(void);
const char* pointops_target_arch(void); /* "gfx950" */
const char* pointops_last_error(void);

/*
 * K nearest neighbours -- replaces `_C.knn_points_idx`
 * (reference: csrc/knn/knn.h:59-80, CPU semantics csrc/knn/knn_cpu.cpp:13-69).
 *   p1 (N,P1,D), p2 (N,P2,D), lengths1 (N,), lengths2 (N,), norm in {1,2}, K >= 1.
 *   idxs (N,P1,K) int64 and dists (N,P1,K) fp32: for each query the K smallest
 *   (dist, idx) pairs in ascending lexicographic order; rows >= lengths1[n] and
 *   slots >= lengths2[n] are 0 / 0.0f.  Distances are unfused fp32
 *   ((dx*dx + dy*dy) + dz*dz), i.e. bit-equal to the reference CPU path.
 *   `version` is accepted for signature compatibility (reference: knn.h:45-57):
 *   -1 = auto; 0..3 select a kernel family when valid, exactly like the reference
 *   they never change results.
 *   workspace: pointops_knn_workspace_bytes() bytes of device scratch (may be NULL
 *   when that returns 0).
 */
size_t pointops_knn_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D,
                                    int64_t K, int version);
int pointops_knn_points_idx(const float* p1, const float* p2, const int64_t* lengths1,
                            const int64_t* lengths2, int64_t N, int64_t P1, int64_t P2,
                            int64_t D, int norm, int64_t K, int version, int64_t* idxs,
                            float* dists, void* workspace, size_t workspace_bytes,
                            void* stream);

/*
 * Read-only view of the dispatch (tests, tools): the kernel family a pointops_knn_points_idx call of this shape and
 * `version` takes and the number of p2 slices it scans (1 = none; > 1: partial lists merged by a second launch),
 * debug knobs included.  Launches nothing, needs no device, changes no choice.  HOST pointers; returns POINTOPS_OK.
 *   *family: 0 nothing to search (N or P1 = 0), 1 grid-pruned search, 2 LDS-transposed queries (any D; register
 *            lists up to K = 32, 64-slot register lists to 64, LDS lists above), 3 plain generic kernel,
 *            4 one wave per query, 5 register scan, one lane per query.
 */
#define POINTOPS_KNN_FAMILY_NONE 0
#define POINTOPS_KNN_FAMILY_GRID 1
#define POINTOPS_KNN_FAMILY_WIDE 2
#define POINTOPS_KNN_FAMILY_GENERIC 3
#define POINTOPS_KNN_FAMILY_SMALL 4
#define POINTOPS_KNN_FAMILY_SCAN 5
int pointops_knn_plan(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K, int version, int* family,
                      int* splits);

/*
 * The same operator REUSING the cell grid a previous call left in `workspace` (the grid-pruned family only:
 * pointops_knn_uses_grid(...) != 0 for the shape; other families ignore `reuse`).  The reference has no counterpart --
 * its operator (csrc/knn/knn.h:59-66) is stateless -- so this is an extension for callers that query the same target
 * cloud repeatedly (chamfer against a fixed ground truth, knn_points followed by more queries of the same cloud):
 *   reuse = 0  build everything (= pointops_knn_points_idx);
 *   reuse = 1  p2, lengths2, N, P1, P2, D, K and version are those of the previous call into this workspace and the
 *              bytes of p2 / lengths2 are unchanged: the bounding boxes, cell tables, the sort of p2 and its refined
 *              cells are reused, only the queries are sorted;
 *   reuse = 2  p1 and lengths1 are unchanged too: no build pass runs at all.
 * The caller vouches for these conditions; results equal reuse = 0 bit for bit when they hold.
 */
int pointops_knn_uses_grid(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K, int version);
int pointops_knn_points_idx_reuse(const float* p1, const float* p2, const int64_t* lengths1,
                                  const int64_t* lengths2, int64_t N, int64_t P1, int64_t P2, int64_t D,
                                  int norm, int64_t K, int version, int64_t* idxs, float* dists,
                                  void* workspace, size_t workspace_bytes, int reuse, void* stream);

/*
 * Diagnostics for the grid-pruned KNN family (version 3): after a pointops_knn_points_idx
 * call that used `workspace`, copies the per-cloud number of queries that the pruning
 * bound could not certify (and that were answered by the whole-cloud scan instead) into
 * counts (2,N) int32 on the device: row 0 = queries re-searched wave-per-query on a growing
 * cell cube, row 1 = queries that ended in the whole-cloud scan.  Stream-ordered, no sync.
 */
int pointops_knn_grid_fallback_counts(const void* workspace, int64_t N, int64_t P1, int64_t P2,
                                      int64_t K, int32_t* counts, void* stream);

/*
 * Diagnostics, same contract: stats (N,14) int32 on the device = cells per dimension G[0..2], cell count,
 * 1 if the cloud was searched through a grid, queries uncertified after the lane pass / after the quad and box passes /
 * sent to the whole-cloud scan, queries deferred to the box search, refined cells, bins of the point sort / of the
 * query sort, crowded bins of the point sort / of the query sort.  (No reference counterpart; used by tools/ and the
 * distribution benchmarks.)
 */
int pointops_knn_grid_stats(const void* workspace, int64_t N, int64_t P1, int64_t P2, int64_t K,
                            int32_t* stats, void* stream);

/* Replaces `_C.knn_check_version` (reference: csrc/knn/knn.h:161, knn.cu:292-303). */
int pointops_knn_check_version(int version, int64_t D, int64_t K);

/*
 * KNN backward -- replaces `_C.knn_points_backward`
 * (reference: csrc/knn/knn.h:127-149, csrc/knn/knn_cpu.cpp:75-128).
 *   grad_p1 (N,P1,D) is a per-query sum over k in k order (deterministic, equal to
 *   the CPU order); grad_p2 (N,P2,D) is a scatter-add (fp32 atomics, order-dependent
 *   last bits, like the reference CUDA path csrc/knn/knn.cu:514-515,538).
 *   Skips k >= min(lengths2[n], K), i >= lengths1[n] and idx == -1.
 */
int pointops_knn_points_backward(const float* p1, const float* p2, const int64_t* lengths1,
                                 const int64_t* lengths2, const int64_t* idxs,
                                 const float* grad_dists, int64_t N, int64_t P1, int64_t P2,
                                 int64_t D, int64_t K, int norm, float* grad_p1,
                                 float* grad_p2, void* stream);

/*
 * Ball query -- replaces `_C.ball_query`
 * (reference: csrc/ball_query/ball_query.h:62-93, ball_query_cpu.cpp:12-54).
 *   First K points of p2 (index order) with dist2 < radius*radius (fp32 product,
 *   strict); idxs padded with -1, dists with 0.
 *   With a `workspace` of pointops_ball_query_workspace_bytes() (0 = not useful for the shape;
 *   workspace may then be NULL) clouds whose balls are SPARSE are answered through a cell grid
 *   instead of the index-order scan; the choice is made per cloud on the device and never changes
 *   results.  Without workspace every cloud is scanned.
 */
size_t pointops_ball_query_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K);
int pointops_ball_query(const float* p1, const float* p2, const int64_t* lengths1,
                        const int64_t* lengths2, int64_t N, int64_t P1, int64_t P2, int64_t D,
                        int64_t K, float radius, int64_t* idxs, float* dists, void* workspace,
                        size_t workspace_bytes, void* stream);

/*
 * Farthest point sampling -- replaces `_C.sample_farthest_points`
 * (reference: csrc/sample_farthest_points/sample_farthest_points.h:55-76,
 *  sample_farthest_points_cpu.cpp:14-103).
 *   points (N,P,D), lengths (N,), K (N,), start_idxs (N,), out idxs (N,max_K) int64
 *   padded with -1 beyond min(lengths[n], K[n]).  max_K = max(K) is passed by the
 *   host (the reference reads it with a host sync: sample_farthest_points.cu:132).
 *   workspace: pointops_fps_workspace_bytes(N, P, max_K) bytes of device scratch (running
 *   min-distance array of the single-workgroup kernel + the per-iteration exchange slots of
 *   the multi-workgroup cluster kernel).
 */
size_t pointops_fps_workspace_bytes(int64_t N, int64_t P, int64_t max_K);
int pointops_sample_farthest_points(const float* points, const int64_t* lengths,
                                    const int64_t* K, const int64_t* start_idxs, int64_t N,
                                    int64_t P, int64_t D, int64_t max_K, int64_t* idxs,
                                    void* workspace, size_t workspace_bytes, void* stream);

/*
 * packed <-> padded -- replace `_C.packed_to_padded` / `_C.padded_to_packed`
 * (reference: csrc/packed_to_padded_tensor/packed_to_padded_tensor.h:78-113,
 *  packed_to_padded_tensor_cpu.cpp:11-70).
 *   packed (F,D), first_idxs (B,), padded (B,max_size,D); cloud b owns packed rows
 *   [first_idxs[b], first_idxs[b+1]) (last cloud: F).  Padding is zero-filled; packed
 *   rows owned by no cloud are zero.  Any B < 2^31, like the reference (65536 clouds and
 *   more run as several launches of 65535 clouds).
 */
int pointops_packed_to_padded(const float* packed, const int64_t* first_idxs, int64_t F,
                              int64_t B, int64_t max_size, int64_t D, float* padded,
                              void* stream);
int pointops_padded_to_packed(const float* padded, const int64_t* first_idxs, int64_t F,
                              int64_t B, int64_t max_size, int64_t D, float* packed,
                              void* stream);

/*
 * Neighbour gather -- the device half of `knn_gather` / `masked_gather`
 * (reference: functions/knn.py:200-250, functions/utils.py:20-65).
 *   x (N,M,U), idx (N,L,K) -> out (N,L,K,U) with out[n,l,k,:] = x[n, idx[n,l,k], :];
 *   zero where k >= lengths[n] (lengths may be NULL) or idx < 0.
 * Backward: grad_x (N,M,U) += scatter of grad_out with the same masks (fp32 atomics);
 *   grad_x is zero-filled by the call.
 */
int pointops_gather_neighbors(const float* x, const int64_t* idx, const int64_t* lengths,
                              int64_t N, int64_t M, int64_t U, int64_t L, int64_t K,
                              float* out, void* stream);
int pointops_gather_neighbors_backward(const float* grad_out, const int64_t* idx,
                                       const int64_t* lengths, int64_t N, int64_t M,
                                       int64_t U, int64_t L, int64_t K, float* grad_x,
                                       void* stream);

/*
 * DETERMINISTIC forms of the two scatter backward passes (csrc/backward_det.hip): the neighbour table is inverted
 * with a stable radix sort and every target row sums its addends in table order -- for knn_points_backward the order
 * of the reference's CPU loop (csrc/knn/knn_cpu.cpp:100-125), so grad_p2 is bit-equal to it.  Same arguments and
 * masks as the calls above plus `workspace` of pointops_backward_det_workspace_bytes(N, L, K, M) bytes
 * (knn: L = P1, M = P2; gather: L, M as given).  The neighbour table must have fewer than 2^31 entries.
 * The host wrappers select them under torch.use_deterministic_algorithms(True).
 */
size_t pointops_backward_det_workspace_bytes(int64_t N, int64_t L, int64_t K, int64_t M);
int pointops_knn_points_backward_det(const float* p1, const float* p2, const int64_t* lengths1,
                                     const int64_t* lengths2, const int64_t* idxs,
                                     const float* grad_dists, int64_t N, int64_t P1, int64_t P2,
                                     int64_t D, int64_t K, int norm, float* grad_p1, float* grad_p2,
                                     void* workspace, size_t workspace_bytes, void* stream);
int pointops_gather_neighbors_backward_det(const float* grad_out, const int64_t* idx,
                                           const int64_t* lengths, int64_t N, int64_t M, int64_t U,
                                           int64_t L, int64_t K, float* grad_x, void* workspace,
                                           size_t workspace_bytes, void* stream);

/*
 * Chamfer point-loss reduction -- the fused tail of
 * `_chamfer_distance_single_direction` (reference: functions/chamfer.py:134-185)
 * for point_reduction in {"sum","mean"}:
 *   out[n] = (sum_{i < lengths[n]} dists[n,i]) * (weights ? weights[n] : 1)
 *            / (mean ? max(lengths[n],1) : 1)
 *   dists (N,P) are the K=1 KNN distances.  Summation order is a fixed tree per
 *   cloud (deterministic), compared with the reference at 1e-5 relative.
 */
int pointops_chamfer_reduce(const float* dists, const int64_t* lengths, const float* weights,
                            int64_t N, int64_t P, int mean, float* out, void* stream);

/*
 * Fused single-direction chamfer terms for K = 1 and point_reduction in {"sum","mean"} --
 * the tail of `_chamfer_distance_single_direction` after its knn_points call
 * (reference: functions/chamfer.py:135-185) including the per-feature cosine loss:
 *   out[0][n]   = w_n / den_n * sum_{i < xlen_n} dists[n,i]
 *   out[1+f][n] = w_n / den_n * sum_{i < xlen_n} (1 - |cos(xf_f[n,i], yf_f[n, idx[n,i]])|)   (|.| if abs_cosine)
 * with den_n = max(xlen_n, 1) for "mean", 1 for "sum"; cos uses F.cosine_similarity's eps = 1e-6.
 * x_feats / y_feats / C are HOST arrays of F (<= 4) device pointers / channel counts (<= 16).
 * The backward is closed-form: grad_x, grad_x_feats written densely, grad_y / grad_y_feats are
 * zero-filled then scatter-added with fp32 atomics.  grad_out is (1+F, N).
 * Any N < 2^31 in every chamfer entry, the pair entries below included (65536 clouds and more run as several launches
 * of 65535 clouds over the same buffers; the workspace sizes are those of the whole batch).
 */
size_t pointops_chamfer_workspace_bytes(int64_t N, int64_t P1);
int pointops_chamfer_forward(const float* dists, const int64_t* idx, const int64_t* x_lengths,
                             const int64_t* y_lengths, const float* weights, int64_t N, int64_t P1,
                             int64_t P2, int F, const float* const* x_feats, const float* const* y_feats,
                             const int64_t* C, int abs_cosine, int mean, float* out, void* workspace,
                             size_t workspace_bytes, void* stream);
int pointops_chamfer_backward(const float* x, const float* y, const int64_t* idx, const int64_t* x_lengths,
                              const int64_t* y_lengths, const float* weights, const float* grad_out,
                              int64_t N, int64_t P1, int64_t P2, int64_t D, int norm, int F,
                              const float* const* x_feats, const float* const* y_feats, const int64_t* C,
                              int abs_cosine, int mean, float* grad_x, float* grad_y,
                              float* const* grad_x_feats, float* const* grad_y_feats, void* stream);
/*
 * The same gradients ADDED to buffers that already hold gradients (no reference counterpart: the reference sums the
 * two directions of a bidirectional chamfer distance through autograd).  After pointops_chamfer_backward for the
 * direction x -> y, the direction y -> x calls this with the roles swapped -- (x, y) := (y, x), grad_x := the first
 * call's grad_y, grad_y := its grad_x, likewise the feature gradients: the dense query-side terms are added element
 * by element, the target-side terms by the same fp32 atomics, nothing is zero-filled.
 */
int pointops_chamfer_backward_accumulate(const float* x, const float* y, const int64_t* idx,
                                         const int64_t* x_lengths, const int64_t* y_lengths, const float* weights,
                                         const float* grad_out, int64_t N, int64_t P1, int64_t P2, int64_t D,
                                         int norm, int F, const float* const* x_feats, const float* const* y_feats,
                                         const int64_t* C, int abs_cosine, int mean, float* grad_x, float* grad_y,
                                         float* const* grad_x_feats, float* const* grad_y_feats, void* stream);

/*
 * BOTH directions of an unweighted chamfer distance with point_reduction in {"sum","mean"} behind one entry (no
 * reference counterpart; the composition of `chamfer_distance`, reference: functions/chamfer.py:188-312, for
 * weights=None): the K=1 searches x -> y and y -> x (pointops_knn_points_idx), pointops_chamfer_forward on each, the
 * sum of the two directions and the batch reduction.
 *   batch_reduction: 0 = None -> each of the 1+F outputs is (N,);  1 = "mean", 2 = "sum" -> each is one float
 *   outs: HOST array of 1+F device pointers (the point term, then one per feature pair)
 *   idx_xy (N,P1), idx_yx (N,P2): the neighbour indices, outputs, needed by the backward.
 * The backward takes 1+F gradient pointers (HOST array; a null entry is a zero gradient; each points to one float
 * after a batch reduction, to N floats without one) and writes grad_x, grad_y, grad_x_feats, grad_y_feats
 * (every element written: no pre-zeroing needed); workspace: pointops_chamfer_pair_backward_workspace_bytes(N, F), the
 * (1+F)*N floats of the per-cloud output gradients.
 */
size_t pointops_chamfer_pair_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int F);
size_t pointops_chamfer_pair_backward_workspace_bytes(int64_t N, int F);
int pointops_chamfer_pair_forward(const float* x, const float* y, const int64_t* x_lengths,
                                  const int64_t* y_lengths, int64_t N, int64_t P1, int64_t P2, int64_t D, int norm,
                                  int F, const float* const* x_feats, const float* const* y_feats, const int64_t* C,
                                  int abs_cosine, int mean, int batch_reduction, int64_t* idx_xy, int64_t* idx_yx,
                                  float* const* outs, void* workspace, size_t workspace_bytes, void* stream);
int pointops_chamfer_pair_backward(const float* x, const float* y, const int64_t* idx_xy, const int64_t* idx_yx,
                                   const int64_t* x_lengths, const int64_t* y_lengths, const float* const* grads,
                                   int64_t N, int64_t P1, int64_t P2, int64_t D, int norm, int F,
                                   const float* const* x_feats, const float* const* y_feats, const int64_t* C,
                                   int abs_cosine, int mean, int batch_reduction, float* grad_x, float* grad_y,
                                   float* const* grad_x_feats, float* const* grad_y_feats, void* workspace,
                                   size_t workspace_bytes, void* stream);

/*
 * Inverse-CDF sampling -- replaces `_C.sample_pdf` (reference: csrc/sample_pdf/sample_pdf.h:58-78,
 * CPU semantics sample_pdf_cpu.cpp:19-99, the USE_BINARY_SEARCH build).
 *   bins (batch, n_bins+1), weights (batch, n_bins), outputs (batch, n_samples) holding the quantiles
 *   u in [0,1] on entry and the samples on return (in place, like the reference).
 */
int pointops_sample_pdf(const float* bins, const float* weights, float* outputs, int64_t batch,
                        int64_t n_bins, int64_t n_samples, float eps, void* stream);

/*
 * Per-point covariance of a gathered K-neighbourhood, fused -- device half of get_point_covariances
 * (reference: functions/utils.py:111-153, which materialises a (N,P,K,D,D) tensor).
 *   knn (N,P,K,D) fp32 -> cov (N,P,D,D): cov[a][b] = mean_k (x_k[a]-m[a])(x_k[b]-m[b]), m = mean_k x_k.
 *   backward: grad_knn (N,P,K,D) = (G + G^T)(x_k - m) / K for G = grad_cov (N,P,D,D).  1 <= D <= 8.
 */
int pointops_point_covariances(const float* knn, int64_t N, int64_t P, int64_t K, int64_t D, float* cov,
                               void* stream);
int pointops_point_covariances_backward(const float* knn, const float* grad_cov, int64_t N, int64_t P, int64_t K,
                                        int64_t D, float* grad_knn, void* stream);

/*
 * Per-point curvatures and local coordinate frames of a K-neighbourhood, fused -- device half of
 * estimate_pointcloud_local_coord_frames / estimate_pointcloud_normals (PyTorch3D's ops/points_normals.py; the
 * reference package has only the covariance, functions/utils.py:111-153, and leaves the rest to torch).
 *   points (N,P,3) fp32, lengths (N,), idx (N,P,K) int64 (knn_points of points against itself), K >= 1.
 *   For every row i < lengths[n]: the neighbours x_k = points[n, idx[n,i,k]] (zero where k >= lengths[n] or idx is
 *   outside [0,P)), C = mean_k (x_k - m)(x_k - m)^T with m = mean_k x_k -- bit-equal to pointops_point_covariances
 *   of pointops_gather_neighbors(points, idx, lengths) --, then its eigen-decomposition (fp64 cyclic Jacobi, rounded
 *   to fp32): curvatures (N,P,3) = eigenvalues ascending, frames (N,P,3,3) with column j = unit eigenvector j.
 *   disambiguate != 0: columns 0 (n) and 2 (z) are negated when fewer than K/2 neighbours have (x_k - x_i).v > 0
 *   (x_i = points[n,i]), and column 1 becomes n x z.  Otherwise the eigenvector signs are implementation-defined.
 *   Rows i >= lengths[n] are zero in both outputs; a zero C gives zero curvatures and the identity frame (before
 *   disambiguation).  No atomics (deterministic), no workspace.  N < 65536 (a bigger batch is POINTOPS_EINVAL:
 *   nothing is launched, no output is written); the backward below has no such limit.
 * Backward: grad_cov (N,P,3,3) from the saved outputs and their gradients (N,P,3), (N,P,3,3) -- with disambiguate,
 *   y = n x z is folded into n and z first; then grad_C = sum_i g_i v_i v_i^T
 *   + sum_{i != j} (v_j . grad_v_i) / (lambda_i - lambda_j) v_j v_i^T.  Rows i >= lengths[n] get 0.  Coincident
 *   eigenvalues divide by zero (inf / nan), as torch.linalg.eigh's backward does.  The gradient of the points follows
 *   through pointops_gather_neighbors, pointops_point_covariances_backward and pointops_gather_neighbors_backward.
 */
int pointops_local_frames(const float* points, const int64_t* lengths, const int64_t* idx, int64_t N, int64_t P,
                          int64_t K, int disambiguate, float* curvatures, float* frames, void* stream);
int pointops_local_frames_backward(const float* curvatures, const float* frames, const float* grad_curvatures,
                                   const float* grad_frames, const int64_t* lengths, int64_t N, int64_t P,
                                   int disambiguate, float* grad_cov, void* stream);

/*
 * Alignment of corresponding points (weighted Umeyama / Kabsch), fused -- device half of PyTorch3D's
 * ops/points_alignment.py `corresponding_points_alignment` (the reference package has no registration at all).
 *   X (N,P,D), Y (N,P2,D) fp32, D in {2,3}; idx (N,P) int64 or NULL: row i of X corresponds to Y[n, idx[n,i]] (clamped
 *   into [0,P2)), without idx to Y[n,i] (then P2 == P); lengths (N,) or NULL (= P); weights (N,P) fp32 or NULL (= 1).
 *   With w_i = weights[n,i] for i < lengths[n] and 0 above, W = max(sum w, eps), xm = sum w x / W, ym likewise,
 *   C = sum w^2 (x - xm)(y - ym)^T / W = U S V^T:  R (N,D,D) = U E V^T with E = diag(1,..,1, det(U V^T)) (E = I when
 *   allow_reflection), s (N,) = tr(E S) / max(sum w^2 |x - xm|^2 / W, eps) when estimate_scale, else 1, and
 *   T (N,D) = ym - s xm R  -- the row-vector convention  X_aligned = s X R + T.
 *   Sums are fp64 and reduced in a fixed order (no atomics: bit-reproducible); the D x D SVD is a one-sided fp64
 *   Jacobi on C itself.  A rank-deficient C (collinear or coincident points, an empty cloud) gives a finite
 *   orthogonal R, the identity for C == 0.
 *   moments (N, 3+4D+D*D) fp64 or NULL: the reduced sums about the pivots X[n,0], Y[n,0] (what the backward needs);
 *   singular_values (N,D) fp32 or NULL: S, descending.  workspace: pointops_points_alignment_workspace_bytes(N,P,D).
 *   N < 65536 in both entries (the cloud is a grid's y coordinate); a bigger batch is POINTOPS_EINVAL, nothing is
 *   launched and no output is written.
 * Backward (without idx): grad_moments (N, 3+4D+D*D) fp64 -> grad_X, grad_Y (N,P,D), grad_weights (N,P) or NULL;
 *   rows i >= lengths[n] get 0.  The gradient of the moments is the host's business (N tiny solves).
 */
size_t pointops_points_alignment_workspace_bytes(int64_t N, int64_t P, int64_t D);
int pointops_points_alignment(const float* X, const float* Y, const int64_t* idx, const int64_t* lengths,
                              const float* weights, int64_t N, int64_t P, int64_t P2, int64_t D, int estimate_scale,
                              int allow_reflection, double eps, float* R, float* T, float* s, double* moments,
                              float* singular_values, void* workspace, size_t workspace_bytes, void* stream);
int pointops_points_alignment_backward(const float* X, const float* Y, const int64_t* lengths, const float* weights,
                                       const double* grad_moments, int64_t N, int64_t P, int64_t D, float* grad_X,
                                       float* grad_Y, float* grad_weights, void* stream);

/*
 * One iteration of PyTorch3D's `iterative_closest_point` behind one entry: the K=1, L2 search of Xt (N,P1,D) in
 * Y (N,P2,D) (pointops_knn_points_idx_reuse, version -1, on `knn_workspace` of pointops_knn_workspace_bytes(N,P1,P2,D,
 * 1,-1) bytes), the alignment of X_init to Y[idx] weighted by the validity mask of lengths_x (eps 1e-9), Xt = s X_init R
 * + T (fp32; rows >= lengths_x[n] zero) written IN PLACE over the queries, and
 *   rmse[n] = sqrt(sum_valid |Xt - Y[idx]|^2 / max(lengths_x[n], 1e-9))       (in/out: the previous iteration's on entry -- not
 *   used when `first` != 0, so the first call may pass an uninitialised buffer --, this one's on return)
 *   converged[0] = 1 when (prev - rmse) / prev <= relative_rmse_thr for every cloud, else 0; the change counts as 1
 *   when `first` != 0 and as 0 where prev == 0 (an empty or exactly matched cloud has nothing left to gain).
 *   reuse: 0 = build the search structure; 1 = the caller vouches that Y, lengths_y and the shape are those of the
 *   previous call into knn_workspace (see pointops_knn_points_idx_reuse); -1 = no search, idx (N,P1) is an input.
 *   idx (N,P1) int64 and dists (N,P1) fp32 are outputs of the search; R, T, s as above.  N, P1, P2 >= 1.
 *   workspace: pointops_icp_workspace_bytes(N, P1, D).  Nothing synchronises; no floating-point atomics.
 *   N < 65536, as for pointops_points_alignment.
 */
size_t pointops_icp_workspace_bytes(int64_t N, int64_t P1, int64_t D);
int pointops_icp_iteration(const float* X_init, float* Xt, const float* Y, const int64_t* lengths_x,
                           const int64_t* lengths_y, int64_t N, int64_t P1, int64_t P2, int64_t D, int estimate_scale,
                           int allow_reflection, int first, int reuse, float relative_rmse_thr, int64_t* idx,
                           float* dists, float* R, float* T, float* s, float* rmse, int32_t* converged,
                           void* knn_workspace, size_t knn_workspace_bytes, void* workspace, size_t workspace_bytes,
                           void* stream);

/*
 * REGISTRATION.  One step of registration_icp -- trimmed point-to-plane or point-to-point ICP (Open3D's
 * registration_icp with a mandatory max_correspondence_distance; PCL's IterativeClosestPoint with
 * setMaxCorrespondenceDistance) -- device half of functions/registration.py.  The semantics are this library's own.
 * float32, three dimensions, rigid motion only; the row-vector convention x -> x R + T throughout.
 *   X_init (N,P1,3), Y (N,P2,3), target_normals (N,P2,3) fp32 (NULL allowed for point to point; used as given, never
 *   renormalised), lengths_x, lengths_y (N,) (clamped into [0,P]); 1 <= N < 65536, P1, P2 >= 1.
 *   R_init (N,3,3), T_init (N,3) fp32 or NULL (the identity): read only when `first` != 0.
 * Per cloud the run keeps, in buffers the caller owns and passes to every step:
 *   state (N,16) fp64: the accumulated transform R (9, row-major), T (3), prev_fitness, prev_rmse, 2 spare words;
 *   status (N,) int32: 2 = running, 0 = frozen, converged, 1 = frozen, degenerate;  iterations (N,) int32: updates
 *   applied;  Xt (N,P1,3) fp32: the transformed cloud, the queries of the search.
 * `first` != 0 (step i = 0) initialises all of them (they may be uninitialised on entry): state from R_init / T_init,
 * status 2, iterations 0, Xt = X_init R_init + T_init in the fp32 arithmetic of step 7.
 * Step i, for every cloud with status 2 (a frozen cloud leaves everything as it is: see step 7):
 *   1. Search: idx (N,P1) int64, dists (N,P1) fp32 = the K=1, L2 pointops_knn_points_idx_reuse of Xt in Y on
 *      `knn_workspace` (pointops_knn_workspace_bytes(N,P1,P2,3,1,search_version) bytes).  search_version is what
 *      pointops_registration_search_version() returned when the run began (-1, the search's own choice of kernel family
 *      by shape, unless a debug knob forces the grid; it never changes results): a run asks once and passes the same
 *      value to every step, since the workspace built by step 0 belongs to one family.  reuse: 0 = build the search structure,
 *      1 = the caller vouches that Y, lengths_y and the shape are those of the previous call into knn_workspace.
 *      d2 = dists[n,r], j = idx[n,r].  (The search runs for the whole batch; a frozen cloud's rows come out unchanged.)
 *      search_version == POINTOPS_REGISTRATION_SEARCH_BOUNDED (no version of knn_points) asks for the BOUNDED search
 *      instead: the K=1 pointops_knn_in_radius of Xt in Y with radius = max_correspondence_distance, on a
 *      `knn_workspace` of pointops_knn_in_radius_workspace_bytes(N,P1,P2,3,1) bytes, with the same `reuse`.  Then idx,
 *      dists hold (-1, 0) on every row with no neighbour inside the radius, and the exact search's values elsewhere.
 *   2. Inliers: row r is an inlier iff r < lengths_x[n], lengths_y[n] > 0, j >= 0 and d2 < fl32(
 *      max_correspondence_distance * max_correspondence_distance) -- ball_query's rule (the exact search never gives
 *      j < 0 where lengths_y[n] > 0; the bounded search gives it exactly where d2 < r2 fails, so both searches give
 *      the same inliers and every later step the same bytes).  correspondences[n,r] = j for an inlier, else -1.
 *   3. Evaluation: c = the number of inliers, fitness = fl32(c / max(lengths_x[n], 1)) and
 *      inlier_rmse = fl32(sqrt(sum d2 / max(c, 1))) with the sum and the quotients in fp64: they describe the transform
 *      in effect at the search.  num_correspondences[n] = c.
 *   4. If i > 0 and |fitness - prev_fitness| < relative_fitness and |inlier_rmse - prev_rmse| < relative_rmse (fp64
 *      differences of the fp32 values; Open3D's absolute differences despite the names): status = 0.  In every case
 *      prev_fitness = fitness and prev_rmse = inlier_rmse afterwards.
 *   5. Otherwise, when `update` != 0:
 *      estimation 1, point to plane: with the pivot c0 = Xt[n,0] and, per inlier, p = Xt - c0, q = Y[j],
 *        n = target_normals[j], rho = (Xt - q).n, J = [p x n, n] (all fp64 from the fp32 values):  A = sum J^T J (the 21
 *        entries of its upper triangle, row by row), b = -sum J rho.  A x = b by an fp64 Cholesky, x = (alpha, beta,
 *        gamma, t);  Rd = (Rz(gamma) Ry(beta) Rx(alpha))^T, built from the sines and cosines, not linearised;
 *        R <- R Rd and T <- (T - c0) Rd + c0 + t.
 *      estimation 0, point to point: (R, T) <- pointops_points_alignment's solve of the ORIGINAL rows X_init onto Y[j]
 *        with weight 1 on inliers and 0 elsewhere (the 24 moments about the pivots X_init[n,0], Y[n,0]; eps 1e-9, no
 *        scale, no reflection).
 *      iterations += 1.
 *   6. Instead of 5, status = 1 and the transform stays as it is when c < 6 (point to plane) or c < 3 (point to
 *      point), or when a Cholesky pivot -- the diagonal entry of row j after the eliminations of the rows before it --
 *      is not greater than kIcpDegeneratePivot = 1e-10 times the ORIGINAL diagonal entry of that row.  A definition,
 *      not a measurement; one plane as the target (rank 3) trips it.
 *   7. R (N,3,3), T (N,3) = fl32 of the accumulated transform, fitness (N,), inlier_rmse (N,): this step's history
 *      entry, written for EVERY cloud (a frozen one repeats its last entry).  With `update` != 0, every cloud that step
 *      5 moved gets Xt = X_init R + T from those fp32 values, v = ((x0 R[0][k] + x1 R[1][k]) + x2 R[2][k]) + T[k],
 *      unfused; rows >= lengths_x[n] are zero.
 *   all_frozen[0] = 1 when no cloud has status 2 after the step, else 0.
 *   moments (N,35) fp64 or NULL, for tests: the reduced sums of the step -- point to plane: A (21), b (6), c, sum d2;
 *   point to point: the 24 moments of pointops_points_alignment, three zeros, c, sum d2 -- and, in words 29..34, the x =
 *   (alpha, beta, gamma, t) that step 5's Cholesky solved (zeros for point to point and wherever step 5 did not move
 *   the cloud).  All 35 words are zero for a frozen cloud.
 * `update` == 0 is the evaluate-only step (1-4 and 7).  Since a frozen cloud does nothing, enqueueing more steps than
 * a run needs is legal and changes no byte: a host loop may read all_frozen as rarely as it likes, or never.
 * All sums are fp64 in an order fixed by the row index and the launch shape (a function of P1 alone): two calls are
 * byte-equal, and a cloud gives the same bytes alone and inside any batch of the same padded widths.  No
 * floating-point atomics.  workspace: pointops_registration_workspace_bytes(N, P1).  A short or null workspace of
 * either kind is POINTOPS_EWORKSPACE and nothing is launched.  Nothing synchronises.
 */
#define POINTOPS_REGISTRATION_SEARCH_BOUNDED (-2)
int pointops_registration_search_version(void);
size_t pointops_registration_workspace_bytes(int64_t N, int64_t P1);
int pointops_registration_step(const float* X_init, const float* Y, const float* target_normals,
                               const int64_t* lengths_x, const int64_t* lengths_y, const float* R_init,
                               const float* T_init, int64_t N, int64_t P1, int64_t P2,
                               float max_correspondence_distance, double relative_fitness, double relative_rmse,
                               int estimation, int update, int first, int reuse, int search_version, float* Xt,
                               double* state, int32_t* status, int32_t* iterations, int64_t* idx, float* dists,
                               int64_t* correspondences, int64_t* num_correspondences, float* R, float* T,
                               float* fitness, float* inlier_rmse, int32_t* all_frozen, double* moments,
                               void* knn_workspace, size_t knn_workspace_bytes, void* workspace,
                               size_t workspace_bytes, void* stream);

/*
 * Fast Point Feature Histograms (Rusu et al. 2009; 33 bins per point, three groups of 11) and the point-pair features
 * under them, in two fused passes over a neighbour table -- device half of functions/fpfh.py.  The semantics are this
 * library's own; all arithmetic is unfused fp32 in the order written.
 *   points (N,P,3), normals (N,P,3) fp32 (used as given, never renormalised); idx (N,P,K) int64: the knn_points or
 *   ball_query table of the cloud against itself; lengths (N,) or NULL (= P).  1 <= K <= 255, N < 65536 in both entries (a
 *   bigger batch is POINTOPS_EINVAL: nothing is launched, no output is written).
 *   Live slots: slot k of row i < lengths[n] is live when j = idx[n,i,k] has 0 <= j < lengths[n], j != i and
 *   d2 = dp.dp > 0 for dp = p_j - p_i (ball_query's -1 padding, the self match and exact duplicates are dead).
 *   Pair features of a live slot: d = sqrtf(d2), a1 = n_i.dp / d, a2 = n_j.dp / d.  If |a1| < |a2|: ns = n_j,
 *   nt = n_i, dp = -dp, f3 = -a2; otherwise ns = n_i, nt = n_j, f3 = a1.  v = dp x ns; the slot is COUNTED when it is
 *   live and |v| > 0; then v /= |v|, w = ns x v, f2 = v.nt, f1 = atan2f(w.nt, ns.nt).
 *   pair_features (N,P,K,4), or NULL: (f1, f2, f3, d) of counted slots, zeros for every other slot and row.
 *   Bins: b1 = clamp(floorf((f1 + PI_F) * C1_F), 0, 10) with C1_F = (float)(11 / (2 pi)),
 *   b2 = clamp(floorf((f2 + 1.0f) * 5.5f), 0, 10), b3 likewise from f3; clamped in floating point, so a non-finite
 *   feature lands in a bin.
 *   spfh (N,P,33): with m counted slots in the row, spfh[11 c + b_c] = (float)count * (100.0f / (float)m); all zeros
 *   when m == 0.  Each group of 11 sums to 100 when m > 0.
 * pointops_fpfh: acc[b] = sum over the live slots in k order of spfh[j][b] / d2, S_c = the sum of acc over group c,
 *   fpfh (N,P,33)[b] = (S_c > 0 ? acc[b] * 100 / S_c : 0) + spfh[i][b].
 * Rows i >= lengths[n] are zero in every output.  Outputs are fully written; no workspace, no atomics on global
 * memory, a fixed summation order: results are bit-reproducible.  N == 0 or P == 0 launches nothing.
 */
int pointops_spfh(const float* points, const float* normals, const int64_t* idx, const int64_t* lengths, int64_t N,
                  int64_t P, int64_t K, float* pair_features, float* spfh, void* stream);
int pointops_fpfh(const float* points, const int64_t* idx, const int64_t* lengths, const float* spfh, int64_t N,
                  int64_t P, int64_t K, float* fpfh, void* stream);

/*
 * RANSAC over putative correspondences: the robust estimator between the descriptor matches (mutual nearest
 * neighbours of FPFH rows: mostly wrong on real scans) and pointops_points_alignment / pointops_icp_iteration -- device
 * half of functions/ransac.py.  The semantics are this library's own; all fp32 arithmetic is unfused and in the order
 * written.  float32, three dimensions, proper rotations only (three pairs cannot tell a rotation from a reflection).
 *   X (N,P1,3), Y (N,P2,3) fp32; corr (N,P1) int64 or NULL: row i of X is matched to row corr[n,i] of Y (NULL: to row i,
 *   then P2 == P1); lengths1, lengths2 (N,) or NULL (= P1, P2; clamped into [0,P]); samples_in (N,H,3) int64 or NULL.
 *   1. Valid correspondences: row i of cloud n is VALID when i < lengths1[n] and 0 <= corr[n,i] < lengths2[n].  The
 *      valid rows in ascending order are v[0..M_n); two rows may share a target.
 *   2. Draws (samples_in == NULL and M_n >= 3): with mix(x) = { x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15;
 *      x *= 0x846ca68b; x ^= x >> 16 } on uint32 (lowbias32) and g = first_cloud + n,
 *        hash32(seed, g, h, j) = mix(mix(mix(mix(mix((uint32)seed + 0x9e3779b9) ^ (uint32)(seed >> 32)) ^ g) ^ h) ^ j),
 *      u_j = hash32(seed, g, h, j) for j = 0, 1, 2 and mulhi(a,b) = ((uint64)a * b) >> 32:
 *        i0 = mulhi(u0, M);  i1 = mulhi(u1, M-1), i1 += (i1 >= i0);
 *        i2 = mulhi(u2, M-2), i2 += (i2 >= min(i0,i1)), then i2 += (i2 >= max(i0,i1)).
 *      The triple of hypothesis h is the rows v[i0], v[i1], v[i2]: distinct, uniform.  first_cloud is the index of
 *      cloud 0 of this call in the caller's batch, so a batch cut into several calls draws what one call would.
 *      With samples_in the triple is samples_in[n,h,:] and nothing is drawn.
 *   3. A hypothesis is VALID when its three rows are distinct valid correspondences (only samples_in can violate that;
 *      a cloud with M_n < 3 and no samples_in has none) and, when estimate_scale == 0 and edge_length_ratio > 0, every
 *      pair (a,b) of (0,1), (0,2), (1,2) passes the edge test: with q = ratio * ratio (fp32), dx = x_a - x_b,
 *      lx = (dx0*dx0 + dx1*dx1) + dx2*dx2 and ly likewise from the matched rows of Y:  lx >= q*ly and ly >= q*lx.
 *   4. The transform of a valid hypothesis is pointops_points_alignment of its three pairs with unit weights, eps 1e-9
 *      and no reflection: the moments about pair 0 in fp64, the fp64 solve, one rounding to fp32.  An invalid one has
 *      R = I, T = 0, s = 1 and the count -1.
 *   5. Score: A[j][k] = s * R[j][k] (fp32); for every valid row  r_k = ((x0*A[0][k] + x1*A[1][k]) + x2*A[2][k]) + T[k],
 *      e = r - y, d2 = (e0*e0 + e1*e1) + e2*e2; the row is an inlier iff d2 <= thr2 = inlier_threshold *
 *      inlier_threshold (formed once in fp32).  count = the number of inliers (int32).
 *   6. best[n] = the valid hypothesis with the largest count, the lowest index among equals; -1 when none is valid.
 *   7. Evaluation of a transform: the same formulas give the mask over all P1 rows (0 for rows that are not valid), the
 *      count and rmse = sqrt(sum over the inliers of d2 / max(count, 1)), the sum in fp64 in a fixed order.
 *   8. The winner is evaluated; then, refine_steps times, per cloud and on the device: fit pointops_points_alignment
 *      with idx = corr, weights = the current mask as 0/1, lengths1 and eps 1e-9; evaluate the fit; accept it (transform,
 *      mask, count, rmse) iff its count >= the current count, else keep what is there and ignore the later steps.
 *   9. best[n] == -1 gives R = I, T = 0, s = 1, an all-zero mask, num_inliers 0 and rmse 0.
 *   Outputs: R (N,3,3), T (N,3), s (N,) fp32, inlier_mask (N,P1) one byte 0/1 per row, num_inliers (N,) int64, rmse (N,)
 *   fp32, best (N,) int64; optional (NULL skips them) counts (N,H) int32, hyp_R (N,H,3,3), hyp_T (N,H,3), hyp_s (N,H)
 *   fp32 and samples_out (N,H,3) int64: the rows of X of every triple (-1 where nothing was drawn).  Every output is
 *   fully written.  No atomics, nothing synchronises, nothing is read back: results are bit-reproducible.
 *   workspace: pointops_ransac_workspace_bytes(N, P1, H); a short or null one is POINTOPS_EWORKSPACE with nothing
 *   written.  0 <= N < 65536 (as for pointops_points_alignment, which it calls; a bigger batch goes in slices with
 *   first_cloud), P1 <= 65535 * pointops_ransac_chunk(), P2 < 2^30, 1 <= H <= 2^24, inlier_threshold >= 0,
 *   0 <= edge_length_ratio <= 1, refine_steps >= 0, first_cloud >= 0: anything else is POINTOPS_EINVAL with nothing
 *   launched.  N == 0 launches nothing; P1 == 0 gives the result of (9), whatever corr and P2 are (an empty table has
 *   no address) and without a refit.
 *   pointops_ransac_chunk(): the number of records one scoring workgroup walks (the sizes around which tests probe).
 */
int64_t pointops_ransac_chunk(void);
size_t pointops_ransac_workspace_bytes(int64_t N, int64_t P1, int64_t H);
int pointops_ransac_alignment(const float* X, const float* Y, const int64_t* corr, const int64_t* lengths1,
                              const int64_t* lengths2, const int64_t* samples_in, int64_t N, int64_t P1, int64_t P2,
                              int64_t H, int64_t seed, int64_t first_cloud, float inlier_threshold,
                              float edge_length_ratio, int estimate_scale, int refine_steps, float* R, float* T,
                              float* s, uint8_t* inlier_mask, int64_t* num_inliers, float* rmse, int64_t* best,
                              int32_t* counts, float* hyp_R, float* hyp_T, float* hyp_s, int64_t* samples_out,
                              void* workspace, size_t workspace_bytes, void* stream);

/*
 * DBSCAN / Euclidean clustering: a raw scan cut into objects -- device half of functions/cluster.py.  The semantics
 * are this library's own (they equal scikit-learn's DBSCAN and Open3D's cluster_dbscan except for pairs at exactly
 * eps); all fp32 arithmetic is unfused and in the order written.  Integer outputs only: bit-reproducible.
 *   points (N,P,D) fp32, D in 1..3; lengths (N,) or NULL (= P; clamped into [0,P]).  Per cloud n, over its first
 *   lengths[n] points:
 *   1. r2 = eps * eps (fp32).  d2(i,j) = (dx*dx + dy*dy) + dz*dz over the D coordinates, dx = x_i - x_j: ball query's
 *      expression, symmetric bit for bit.  i and j are NEIGHBOURS iff d2(i,j) < r2 (ball query's comparison); a point
 *      is its own neighbour unless a coordinate is not finite (or r2 underflows to 0).
 *   2. i is a CORE point iff it has at least min_points neighbours, itself included.
 *   3. CLUSTERS: the connected components of the neighbour graph restricted to the core points, numbered 0, 1, ... in
 *      the order of their smallest member index.
 *   4. BORDER: a non-core point with at least one core neighbour takes the smallest label among its core neighbours'
 *      clusters.  NOISE: every other point, and every padding row, gets label -1.
 *   min_points == 1 is Euclidean clustering: the connected components of the radius graph.
 *   Outputs: labels (N,P) int64, num_clusters (N,) int64, core_mask (N,P) one byte 0/1 per row (0 on padding rows).
 *   Every output is fully written.  Nothing synchronises, nothing is read back.
 *   workspace: pointops_cluster_workspace_bytes(N, P); a short or null one is POINTOPS_EWORKSPACE with nothing written.
 *   0 <= N < 65536 (a bigger batch goes in slices), 0 <= P < 2^30, 1 <= D <= 3, eps finite and > 0, min_points >= 1:
 *   anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing; P == 0 writes num_clusters = 0.
 */
size_t pointops_cluster_workspace_bytes(int64_t N, int64_t P);
int pointops_cluster_dbscan(const float* points, const int64_t* lengths, int64_t N, int64_t P, int64_t D, float eps,
                            int64_t min_points, int64_t* labels, int64_t* num_clusters, uint8_t* core_mask,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * ISS keypoints (Intrinsic Shape Signatures, Zhong 2009; Open3D's compute_iss_keypoints, PCL's ISSKeypoint3D with the
 * unweighted scatter matrix): which points of a cloud deserve a descriptor -- device half of functions/iss.py.  The
 * semantics are this library's own; all fp32 and fp64 arithmetic is unfused and in the order written.  Every output is a
 * function of the input alone: the scatter matrix is summed in integers, so the order of the walk never shows.
 *   points (N,P,3) fp32; lengths (N,) or NULL (= P; clamped into [0,P]); rs = salient_radius, rn = non_max_radius.
 *   d2(i,j) = (dx*dx + dy*dy) + dz*dz in fp32, dx = x_i - x_j: ball query's and cluster_dbscan's expression.  For every
 *   row i < lengths[n] of cloud n:
 *   1. SUPPORT.  S_i = { j < lengths[n] : d2(i,j) < fl32(rs * rs) }; i itself is in S_i when its coordinates are
 *      finite.  n_i = |S_i|.
 *   2. INTEGER MOMENTS.  e = the smallest integer with fl32(rs) <= 2^e, s = 2^(19 - e) as a double.  Per coordinate
 *      q = rint(((double)x_j - (double)x_i) * s), round half to even, an integer with |q| <= 2^19 up to rounding.
 *      M1 = sum over S_i of q (x, y, z), M2 = sum of q q^T (xx, xy, xz, yy, yz, zz), in int64: with P <= 2^24 no sum
 *      reaches 2^63.
 *   3. COVARIANCE in fp64:  m_a = (double)M1_a / n_i;  C_ab = ((double)M2_ab / n_i - m_a * m_b) * s^-2.  n_i == 0: C = 0.
 *   4. EIGENVALUES.  sym3_eigen_f64(C) of csrc/small_solvers.h (cyclic Jacobi in fp64), ascending, each rounded once
 *      to fp32: eigenvalues[n,i,:] = (l0, l1, l2).
 *   5. SALIENCY in fp32, from the rounded eigenvalues:  saliency = l0 when  l0 > 2^-20 * l2  and  l1 < gamma_21 * l2  and
 *      l0 < gamma_32 * l1,  else 0.  The first test is the floor: an eigenvalue below the resolution of the integer
 *      moments is rounding, not structure (it also covers supports of fewer than four points).  The other two are
 *      Open3D's quotient tests written as products: no division by zero.
 *   6. NON-MAXIMUM SUPPRESSION.  T_i = { j < lengths[n] : d2(i,j) < fl32(rn * rn) }.  mask[n,i] = 1 iff saliency_i > 0
 *      and |T_i| >= min_neighbors and no j in T_i beats i, where j BEATS i when saliency_j > saliency_i, or
 *      saliency_j == saliency_i and j < i (ties to the lower index; Open3D keeps both ends of an exact tie).
 *   Rows at or past the length: eigenvalues 0, saliency 0, mask 0 (moments 0).
 *   Outputs: eigenvalues (N,P,3) fp32, saliency (N,P) fp32, mask (N,P) one byte 0/1 per row; optional (NULL skips it)
 *   moments (N,P,10) int64 = (n_i, M1[3], M2[6]).  Every output is fully written.  No atomics of its own, nothing
 *   synchronises, nothing is read back: results are bit-reproducible.
 *   workspace: pointops_iss_workspace_bytes(N, P); a short or null one is POINTOPS_EWORKSPACE with nothing written.
 *   0 <= N < 65536 (a bigger batch goes in slices), 0 <= P <= 2^24, both radii and both gammas finite and > 0,
 *   min_neighbors >= 0: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing.
 */
size_t pointops_iss_workspace_bytes(int64_t N, int64_t P);
int pointops_iss_keypoints(const float* points, const int64_t* lengths, int64_t N, int64_t P, float salient_radius,
                           float non_max_radius, float gamma_21, float gamma_32, int64_t min_neighbors,
                           float* eigenvalues, float* saliency, uint8_t* mask, int64_t* moments, void* workspace,
                           size_t workspace_bytes, void* stream);

/*
 * Moving-least-squares smoothing (PCL's MovingLeastSquares at polynomial order 1; the plane fit at the core of APSS /
 * RIMLS): every point is projected onto the plane fitted to its weighted radius neighbourhood, which also yields a
 * normal and a curvature -- device half of functions/mls.py.  The semantics are this library's own; all fp32 and fp64
 * arithmetic is unfused and in the order written.  Every output is a function of the input alone: the weighted moments
 * are summed in integers, so the order of the walk never shows.
 *   points (N,P,3) fp32; lengths (N,) or NULL (= P; clamped into [0,P]); r = radius.
 *   d2(i,j) = (dx*dx + dy*dy) + dz*dz in fp32, dx = x_i - x_j: ball query's expression.  r2 = fl32(r * r).  For every
 *   row i < lengths[n] of cloud n:
 *   1. SUPPORT.  S_i = { j < lengths[n] : d2(i,j) < r2 }; i itself is in S_i when its coordinates are finite and
 *      r2 > 0.  num_neighbors[n,i] = |S_i|.
 *   2. WEIGHT of j in S_i: the compactly supported quartic (1 - d2 / r2)^4 of APSS / RIMLS, in fp32 from the d2 above:
 *      t = d2 / r2 (one correctly rounded IEEE division), u = 1 - t, w = u * u, w = w * w;  then
 *      wq = rint((double)w * 2^12), round half to even: an integer in [0, 4096].
 *   3. INTEGER MOMENTS.  e = the smallest integer with fl32(r) <= 2^e, s = 2^(15 - e) as a double.  Per coordinate
 *      q = rint(((double)x_j - (double)x_i) * s), round half to even, an integer with |q| < 2^15 + 1.
 *      W = sum over S_i of wq, M1 = sum of wq q (x, y, z), M2 = sum of wq q q^T (xx, xy, xz, yy, yz, zz), in int64.
 *      A term is below 2^42 (1 + 2^-13) in magnitude, so with P <= 2^20 no sum reaches 2^63 (csrc/mls_fit.h).
 *   4. FIT in fp64:  m_a = (double)M1_a / W;  delta_a = m_a / s (the weighted mean offset of the support from x_i);
 *      C_ab = ((double)M2_ab / W - m_a * m_b) * s^-2.  W == 0: C = 0, delta = 0.  sym3_eigen_f64(C) of
 *      csrc/small_solvers.h (cyclic Jacobi in fp64) gives the ascending eigenvalues l0 <= l1 <= l2; n is the
 *      eigenvector of l0, its sign such that its component of largest magnitude is positive (ties to the lower axis).
 *   5. STATUS (one byte):  1 when num_neighbors < min_neighbors;  else 2 when the support does not determine a plane,
 *      l1 <= 2^-20 * l2 (a line, a single location, nothing);  else 0.  A row of status 1 or 2 returns its point
 *      unchanged (the same bits), normal 0 and curvature 0.
 *   6. OUTPUT of a row of status 0:  normals[n,i,:] = n^ = fl32(n), and the point moves along THAT vector, so that the
 *      returned point and the returned normal agree to the last bit: in fp64, with n^ widened exactly,
 *      h = (delta_x n^_x + delta_y n^_y) + delta_z n^_z;  points_out[n,i,a] = fl32((double)x_i,a + h * n^_a), rounded
 *      once.  (delta has a part along the surface of up to |x_j - x_i|: with the unrounded n the returned normal
 *      would reproduce the point only to |delta| 2^-24, not to |h| 2^-24.)
 *      curvature[n,i] = fl32(l0 / ((l0 + l1) + l2)).
 *   7. ITERATIONS.  The map points -> points_out is applied `iterations` times, each pass on the points the one before
 *      it wrote (with its own grid, since the points move), alternating between points_out and one workspace buffer;
 *      normals, curvature, num_neighbors, status and moments are those of the last pass.  All passes are enqueued by
 *      this one call.  points_out must not overlap points.
 *   Rows at or past the length: points_out 0, normals 0, curvature 0, num_neighbors 0, status 0 (moments 0).
 *   Outputs: points_out (N,P,3) fp32, normals (N,P,3) fp32, curvature (N,P) fp32, num_neighbors (N,P) int64, status
 *   (N,P) one byte per row; optional (NULL skips it) moments (N,P,10) int64 = (W, M1[3], M2[6]).  Every output is fully
 *   written.  No atomics of its own, nothing synchronises, nothing is read back: results are bit-reproducible, and a
 *   cloud's rows do not depend on what else is in the batch or on the order of its own rows.
 *   workspace: pointops_mls_workspace_bytes(N, P, iterations); a short or null one is POINTOPS_EWORKSPACE with nothing
 *   written.
 *   0 <= N < 65536 (a bigger batch goes in slices), 0 <= P <= 2^20, radius finite and > 0, min_neighbors >= 0,
 *   1 <= iterations <= 65536: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing.
 */
size_t pointops_mls_workspace_bytes(int64_t N, int64_t P, int64_t iterations);
int pointops_mls_smooth(const float* points, const int64_t* lengths, int64_t N, int64_t P, float radius,
                        int64_t min_neighbors, int64_t iterations, float* points_out, float* normals, float* curvature,
                        int64_t* num_neighbors, uint8_t* status, int64_t* moments, void* workspace,
                        size_t workspace_bytes, void* stream);

/*
 * RANSAC plane extraction: the dominant plane of every cloud (floor, road, table, wall) -- Open3D's segment_plane,
 * PCL's SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE -- device half of functions/plane.py.  The
 * semantics are this library's own; all fp32 and fp64 arithmetic is unfused and in the order written.  float32 points,
 * three dimensions.  A plane is (a, b, c, d): the points with a x + b y + c z + d = 0, (a, b, c) a unit normal.
 *   points (N,P,3) fp32; lengths (N,) or NULL (= P; clamped into [0,P]); mask (N,P) one byte per row or NULL;
 *   samples_in (N,H,3) int64 or NULL.
 *   1. Valid rows: row i of cloud n is VALID when i < lengths[n] and mask is NULL or mask[n,i] != 0.  The valid rows in
 *      ascending order are v[0..M_n).
 *   2. Draws (samples_in == NULL and M_n >= 3): hypothesis h takes the rows v[i0], v[i1], v[i2] with (i0, i1, i2) the
 *      three distinct positions of pointops_ransac_alignment's step 2 -- the same hash32(seed, first_cloud + n, h, j),
 *      the same mulhi reductions -- for M = M_n.  first_cloud is the index of cloud 0 of this call in the caller's
 *      batch, so a batch cut into several calls draws what one call would.  With samples_in the triple is
 *      samples_in[n,h,:], rows of the cloud, and nothing is drawn.
 *   3. A hypothesis is INVALID when M_n < 3 (without samples_in), when one of its rows is not valid or two are the same
 *      (only samples_in can do that), or when it fails a test of step 4.
 *   4. The plane of a hypothesis, in fp64 on the three fp32 points p0, p1, p2:  e1 = p1 - p0, e2 = p2 - p0,
 *      c = e1 x e2 with c0 = e1[1]*e2[2] - e1[2]*e2[1], c1 = e1[2]*e2[0] - e1[0]*e2[2], c2 = e1[0]*e2[1] - e1[1]*e2[0];
 *      |v|^2 = (v0*v0 + v1*v1) + v2*v2.  It is invalid unless |c|^2 > (1e-12 * |e1|^2) * |e2|^2 (collinear and
 *      coincident points and NaN fail this) and, with use_axis, unless (c.A)^2 >= (cosm * cosm) * |c|^2, where
 *      c.A = (c0*A0 + c1*A1) + c2*A2, A = (axis_x, axis_y, axis_z) and cosm = cos_max_angle, both fp32 widened to fp64:
 *      the normal lies within max_angle of +-A.  The caller passes A with unit length.  Then n = c / sqrt(|c|^2),
 *      d = -((n0*p0[0] + n1*p0[1]) + n2*p0[2]).  Sign: with use_axis, (n, d) is negated when n.A < 0; without, when the
 *      component of n of largest magnitude (the lowest index among equal magnitudes) is negative.  (n, d) is rounded
 *      once to fp32; a d that is not finite in fp32 makes the hypothesis invalid.  An invalid hypothesis has the plane
 *      (0,0,0,0) and the count -1.
 *   5. Residual of a row (x, y, z) under a plane:  r = ((x*a + y*b) + z*c) + d in fp32; the row is an inlier iff
 *      |r| <= distance_threshold.  The count of a valid hypothesis is the number of inliers among the valid rows (int32).
 *   6. best[n] = the valid hypothesis with the largest count, the lowest index among equals; -1 when none is valid.
 *   7. Evaluation of a plane: the same formulas give the mask over all P rows (0 for rows that are not valid), the count
 *      and rmse = sqrt(sum over the inliers of r*r / max(count, 1)), r*r and the sum in fp64, by block partials in a
 *      fixed order.
 *   8. The winner is evaluated; then, refine_steps times, per cloud and on the device: with the pivot v[0]'s point and
 *      q = p - pivot (fp64), the moments S1 = count, Sq = sum q, Sqq = sum q q^T over the current inliers (fp64 block
 *      partials in a fixed order); centroid m = Sq / S1, covariance Sqq / S1 - m m^T; the eigenvector n of its smallest
 *      eigenvalue (cyclic Jacobi in fp64: sym3_eigen_f64 of csrc/small_solvers.h), d = -n.(pivot + m), the sign rule
 *      of step 4, one rounding to fp32.  The fit is evaluated and accepted (plane, mask, count, rmse) iff its count >=
 *      the current count; else the cloud keeps what it has and ignores the later steps.  A fit from fewer than three
 *      inliers, a fit that is not finite and -- with use_axis -- a fit outside the cone are rejected likewise.
 *   9. best[n] == -1 gives the plane (0,0,0,0), an all-zero mask, num_inliers 0 and rmse 0.
 *   Outputs: planes (N,4) fp32, inlier_mask (N,P) one byte 0/1 per row, num_inliers (N,) int64, rmse (N,) fp32, best
 *   (N,) int64; optional (NULL skips them) counts (N,H) int32, hyp_planes (N,H,4) fp32 and samples_out (N,H,3) int64:
 *   the rows of every triple (-1 where nothing was drawn).  Every output is fully written, P == 0 included.  No
 *   atomics, nothing synchronises, nothing is read back: results are bit-reproducible.
 *   workspace: pointops_plane_workspace_bytes(N, P, H); a short or null one is POINTOPS_EWORKSPACE with nothing written.
 *   0 <= N < 65536 (a bigger batch goes in slices with first_cloud), P <= 65535 * pointops_plane_chunk(),
 *   1 <= H <= 2^24, distance_threshold finite and >= 0, refine_steps >= 0, first_cloud >= 0 and, with use_axis, a unit
 *   axis and 0 <= cos_max_angle <= 1: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing.
 *   pointops_plane_chunk(): the number of records one scoring workgroup walks (the sizes around which tests probe).
 */
int64_t pointops_plane_chunk(void);
size_t pointops_plane_workspace_bytes(int64_t N, int64_t P, int64_t H);
int pointops_segment_plane(const float* points, const int64_t* lengths, const uint8_t* mask, const int64_t* samples_in,
                           int64_t N, int64_t P, int64_t H, int64_t seed, int64_t first_cloud,
                           float distance_threshold, int use_axis, float axis_x, float axis_y, float axis_z,
                           float cos_max_angle, int refine_steps, float* planes, uint8_t* inlier_mask,
                           int64_t* num_inliers, float* rmse, int64_t* best, int32_t* counts, float* hyp_planes,
                           int64_t* samples_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Voxel-grid pooling (Open3D's voxel_down_sample, PCL's VoxelGrid, the grid pooling of point networks): one point --
 * the centroid -- and one mean feature per occupied voxel, and the integer cell coordinates sparse convolutions consume
 * -- device half of functions/voxel.py.  The semantics are this library's own; all fp64 arithmetic is unfused and in the
 * order written.  Every output is a function of the input alone and has the static shape of the input.
 *   points (N,P,3) fp32; lengths (N,) or NULL (= P; clamped into [0,P]); v = voxel_size, finite in fp32 and > 0;
 *   features (N,P,C) fp32 or NULL (C == 0); origin NULL, (3,) (origin_per_cloud == 0) or (N,3) (origin_per_cloud != 0).
 *   1. LIVE ROWS.  Row i of cloud n is live when i < lengths[n] and its three coordinates are finite.  Every other row
 *      belongs to no voxel.
 *   2. ORIGIN per cloud and axis a, in fp64.  With an origin: o_a = (double)origin_a.  Without: Open3D's rule
 *      o_a = (double)min_a - 0.5 * (double)v, min_a the fp32 minimum over the cloud's live rows.
 *   3. CELL.  c_a(x) = floor(((double)x - o_a) / (double)v): a division, monotone in x.
 *   4. EXTENT.  c_lo = c_a(min_a), c_hi = c_a(max_a).  The cloud is REFUSED, status[n] = 1, when on any axis
 *      c_hi - c_lo >= 2^21, or |c_lo| >= 2^31, or |c_hi| >= 2^31 (fp64 comparisons, before any conversion to an integer;
 *      a comparison with a NaN -- a non-finite origin -- refuses).  A refused cloud has no voxels.  Every other cloud,
 *      one without a live row included, has status[n] = 0.
 *   5. VOXELS.  The voxels of a cloud are the distinct cells (c_x, c_y, c_z) of its live rows, numbered 0 .. V-1 in
 *      ascending (c_z, c_y, c_x) order; the members of a voxel are taken in ascending row index.
 *   6. OUTPUTS, padded to P voxel rows; rows >= V, and every row of a refused or empty cloud, hold the fill value.
 *        num_voxels  (N,)     int64  V                                            --
 *        status      (N,)     int32  0, or 1 for a refused cloud                  --
 *        inverse     (N,P)    int64  the voxel of every input row                 -1 (rows that are not live, refused clouds)
 *        counts      (N,P)    int64  members per voxel                            0
 *        first_index (N,P)    int64  the lowest member row of every voxel         -1
 *        coords      (N,P,3)  int64  (c_x, c_y, c_z), relative to the origin      0      (NULL skips it)
 *        centroids   (N,P,3)  fp32   mean of the members' points (7.)             0
 *        pooled      (N,P,C)  fp32   mean of the members' features (7.)           0      (C > 0 only)
 *   7. MEANS.  An fp64 sum of the members' fp32 values divided by the fp64 count and rounded once to fp32.  The sum's
 *      shape depends on the member's position j within the voxel alone: groups of 16 consecutive members, each added one
 *      after the other to +0.0; chunks of 64 consecutive groups, each combined by the aligned pairwise tree (groups 2k
 *      and 2k+1, then pairs of pairs, ...; a missing group counts +0.0); the chunks added one after the other to +0.0.
 *      Features are averaged and not renormalised (Open3D does the same for normals).
 *   Every output is fully written.  No atomics on floating-point data, nothing synchronises, nothing is read back: two
 *   calls are byte-equal, and the call can be captured into a HIP graph.
 *   workspace: pointops_voxel_workspace_bytes(N, P, C); a short or null one is POINTOPS_EWORKSPACE with nothing written.
 *   0 <= N < 65536 (a bigger batch goes in slices), 0 <= P <= 2^24, 0 <= C <= 1024 (C > 0 needs features and pooled),
 *   voxel_size finite and > 0: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing; P == 0
 *   writes num_voxels = 0 and status = 0 only.
 */
size_t pointops_voxel_workspace_bytes(int64_t N, int64_t P, int64_t C);
int pointops_voxel_downsample(const float* points, const int64_t* lengths, const float* features, const float* origin,
                              int origin_per_cloud, int64_t N, int64_t P, int64_t C, float voxel_size,
                              int64_t* num_voxels, int32_t* status, int64_t* inverse, int64_t* counts,
                              int64_t* first_index, int64_t* coords, float* centroids, float* pooled, void* workspace,
                              size_t workspace_bytes, void* stream);

/*
 * Outlier removal: the stray returns of a real sensor taken out before anything else looks at the cloud -- Open3D's
 * remove_radius_outlier / remove_statistical_outlier, PCL's RadiusOutlierRemoval / StatisticalOutlierRemoval -- device
 * half of functions/filters.py (csrc/filters.hip).  The semantics are this library's own; all fp32 and fp64 arithmetic
 * is unfused and in the order written.  Three entries: the two filters and the compaction both end with.
 *
 * COMPACTION (pointops_mask_compact, and the last step of both filters).
 *   mask (N,P) one byte per row, a row is KEPT when its byte is not 0.
 *   1. index[n, 0 .. k_n) = the kept rows of cloud n in ascending order, index[n, k_n .. P) = -1; num_kept[n] = k_n.
 *   A stable two-level scan without atomics: kept rows counted per block of 1024 rows, the counts of a cloud scanned
 *   by one workgroup, every block scattering behind its offset.  It needs no workspace: until its last launch the
 *   block offsets live in the upper halves of index[n, 0 .. ceil(P / 1024)), which that launch overwrites.
 *   index (N,P) int64 and num_kept (N,) int64 are fully written.  0 <= N < 65536 (a bigger batch goes in slices),
 *   0 <= P < 2^30: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing; P == 0 writes
 *   num_kept = 0.
 *
 * RADIUS FILTER (pointops_radius_outlier): keep the rows with enough company.
 *   points (N,P,D) fp32, D in 1..3; lengths (N,) or NULL (= P; clamped into [0,P]).  Per cloud n:
 *   1. r2 = radius * radius (fp32).  d2(i,j) = (dx*dx + dy*dy) + dz*dz over the D coordinates in fp32, dx = x_i - x_j:
 *      ball query's and pointops_cluster_dbscan's expression.
 *   2. c_i = the number of rows j != i, j < lengths[n], with d2(i,j) < r2, for every row i < lengths[n].
 *   3. mask[n,i] = 1 iff c_i >= min_neighbors.  Rows at or past the length: mask 0 (counts 0).
 *   So mask equals pointops_cluster_dbscan's core_mask at eps = radius, min_points = min_neighbors + 1 on every row
 *   whose coordinates are finite (a row with a non-finite coordinate has c_i = 0 here and no neighbours there).
 *   4. index, num_kept: the COMPACTION of mask.
 *   One lane per point walks the 3x3x3 cube of a grid with cells at least 1.001 radius wide under ball query's
 *   certificate (csrc/radius_walk.h), and stops as soon as c_i reaches min_neighbors -- unless counts is given: then
 *   it finishes and writes the exact c_i.  Clouds too small for a grid, refused grids and lanes without the
 *   certificate walk all pairs: which path a lane takes never changes a result.
 *   Outputs: mask (N,P) one byte 0/1 per row, index (N,P) int64, num_kept (N,) int64; optional (NULL skips it) counts
 *   (N,P) int32.  Every output is fully written.  No atomics of its own, nothing synchronises, nothing is read back.
 *   workspace: pointops_radius_outlier_workspace_bytes(N, P); a short or null one is POINTOPS_EWORKSPACE with nothing
 *   written.  0 <= N < 65536 (a bigger batch goes in slices), 0 <= P < 2^30, 1 <= D <= 3, radius finite and > 0,
 *   min_neighbors >= 0: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing; P == 0
 *   writes num_kept = 0.
 *
 * STATISTICAL FILTER (pointops_statistical_outlier): keep the rows whose mean distance to their nearest neighbours
 * is not far above the cloud's.
 *   dists (N,P,K1) fp32: the SQUARED distances of knn_points of the cloud against itself with K = K1, ascending, the
 *   row's own zero distance among them; K1 = nb_neighbors + 1.  lengths (N,) or NULL (= P; clamped into [0,P]).
 *   Per cloud n with len = its length and cnt = min(K1, len):
 *   1. ROW MEAN, for every row i < len.  cnt >= 2:  m_i = fl32( (sum over k < cnt of sqrt((double)dists[n,i,k]))
 *      / (double)(cnt - 1) ), the sum in fp64 in ascending k, starting from +0.0.  The row's own distance adds 0: this
 *      is PCL's mean over the nb_neighbors nearest OTHER points (Open3D's at nb_neighbors = K1 times K1 / (K1 - 1):
 *      the same mask).  cnt < 2: m_i = 0.  A row is FINITE when m_i is; the others take no part in step 2 and get
 *      mask 0.  mean_distance[n,i] = m_i; 0 on rows at or past the length.
 *   2. CLOUD STATISTICS in fp64, two passes.  n_f = the number of finite rows.  S1 = SUM(m_i), mean = S1 / n_f (0 when
 *      n_f == 0); S2 = SUM((m_i - mean) * (m_i - mean)), std = sqrt(S2 / (n_f - 1)) (0 when n_f < 2).  Both SUMs are
 *      taken over the P rows of the cloud, a row that is not finite or at or past the length entering as +0.0, by one
 *      tree whose shape depends on the row index alone -- not on N, the launch, the device or a debug knob:
 *        - row i belongs to chunk i / 4096 and, within it, to lane (i % 4096) % 256;
 *        - every lane adds its rows of the chunk one after the other, in ascending order, to +0.0 (16 additions);
 *        - the 256 lane sums s[0 .. 256) of a chunk are folded by s[t] = s[t] + s[t + h] for t < h, with
 *          h = 128, 64, ..., 1 in turn: the chunk's sum is s[0];
 *        - the chunk sums are added one after the other, in ascending chunk order, to +0.0.
 *   3. THRESHOLD AND MASK.  threshold[n] = fl32(mean + (double)std_ratio * std); mask[n,i] = 1 iff row i is finite and
 *      m_i <= threshold[n], an fp32 comparison: a lattice whose m_i are all equal keeps every row.
 *   4. index, num_kept: the COMPACTION of mask.
 *   Outputs: mean_distance (N,P) fp32, stats (N,3) fp64 = (mean, std, n_f), threshold (N,) fp32, mask (N,P) one byte
 *   0/1 per row, index (N,P) int64, num_kept (N,) int64.  Every output is fully written.  No atomics, nothing
 *   synchronises, nothing is read back: two calls are byte-equal, a cloud gives the same rows alone and in a batch.
 *   The row formula, the finite test, std and threshold are csrc/filter_stats.h, host and device code.
 *   workspace: pointops_statistical_outlier_workspace_bytes(N, P); a short or null one is POINTOPS_EWORKSPACE with
 *   nothing written.  0 <= N < 65536 (a bigger batch goes in slices), 0 <= P <= 2^24, 2 <= K1 <= 128, std_ratio finite
 *   and >= 0: anything else is POINTOPS_EINVAL with nothing launched.  N == 0 launches nothing; P == 0 writes stats =
 *   (0, 0, 0), threshold = 0 and num_kept = 0.
 */
int pointops_mask_compact(const uint8_t* mask, int64_t N, int64_t P, int64_t* index, int64_t* num_kept, void* stream);
size_t pointops_radius_outlier_workspace_bytes(int64_t N, int64_t P);
int pointops_radius_outlier(const float* points, const int64_t* lengths, int64_t N, int64_t P, int64_t D, float radius,
                            int64_t min_neighbors, uint8_t* mask, int32_t* counts, int64_t* index, int64_t* num_kept,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t pointops_statistical_outlier_workspace_bytes(int64_t N, int64_t P);
int pointops_statistical_outlier(const float* dists, const int64_t* lengths, int64_t N, int64_t P, int64_t K1,
                                 float std_ratio, float* mean_distance, double* stats, float* threshold, uint8_t* mask,
                                 int64_t* index, int64_t* num_kept, void* workspace, size_t workspace_bytes,
                                 void* stream);

/*
 * KNN IN RADIUS: the K nearest points among those closer than a radius, sorted by distance -- Open3D's
 * search_hybrid_vector_3d, PCL's radiusSearch with max_nn on sorted results -- device half of
 * functions/knn_in_radius.py (csrc/knn_in_radius.hip, radius_knn_kernel.h).  The semantics are this library's own.
 *   p1 (N,P1,D), p2 (N,P2,D) fp32, D in 1..3; lengths1, lengths2 (N,) or NULL (= P; clamped into [0,P]).
 *   1. r2 = fl32(radius * radius).  d2(i,j) = ((dx*dx) + dy*dy) + dz*dz over the D coordinates in unfused fp32,
 *      dx = p1[n,i] - p2[n,j]: ball query's expression, the one pointops_knn_points_idx matches bit for bit.
 *   2. The CANDIDATES of row i < lengths1[n] are the rows j < lengths2[n] with d2(i,j) < r2 -- ball query's rule.  A
 *      NaN d2 fails the comparison: such a row is never a neighbour.  d2 == r2 is outside.
 *   3. The result is the first min(K, #candidates) candidates in ascending (d2, j) order: a tie goes to the lower
 *      index.  idxs[n,i,k] = j and dists[n,i,k] = d2 for those, then -1 and 0; counts[n,i] = their number.
 *   4. Rows i >= lengths1[n]: -1, 0, count 0.
 *   On finite inputs this is pointops_knn_points_idx(K, L2) with every slot whose distance is not below r2, or whose
 *   position k >= lengths2[n], turned into padding.
 *   Outputs: idxs (N,P1,K) int64, dists (N,P1,K) fp32; optional (NULL skips it) counts (N,P1) int32.  Every output is
 *   fully written; the buffers may arrive uninitialised.
 *   One lane per query.  The target's grid has cells at least 1.001 radius wide; a lane whose 3x3x3 cube is proven to
 *   contain its ball (every point outside it has a computed d2 >= r2: the face bound of the KNN search) walks the cube,
 *   any other lane -- no certificate, a grid refused for its cloud (non-finite coordinates, cell caps), a call too
 *   small for a grid -- scans its cloud in index order with the same comparison.  Both keep the K smallest 64-bit keys
 *   (d2 bits << 32 | j), whose order is the (d2, j) order (csrc/knn_radius_list.h, host and device code): which path a
 *   lane takes depends on the input alone and changes no byte.  No atomics on results, nothing synchronises, nothing
 *   is read back: two calls are byte-equal, a cloud gives the same rows alone and in a batch.
 *   reuse: 0 = build both sides of the search structure; 1 = the caller vouches that p2, lengths2 and the shape are
 *   those of the previous call into this workspace, and the radius no larger than that call's (the cells stay wide
 *   enough; the certificate is taken per call from this call's r2): only the query side is rebuilt.
 *   workspace: pointops_knn_in_radius_workspace_bytes(N, P1, P2, D, K); a short or null one is POINTOPS_EWORKSPACE with
 *   nothing launched.  0 <= N < 65536 (a bigger batch goes in slices), 0 <= P1 < 2^30, 0 <= P2 <= the grid KNN's
 *   largest cloud, 1 <= D <= 3, 1 <= K <= 64, radius finite and > 0, reuse 0 or 1: anything else is POINTOPS_EINVAL
 *   with nothing launched.  N == 0 and P1 == 0 launch nothing.
 */
size_t pointops_knn_in_radius_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K);
int pointops_knn_in_radius(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                           int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K, float radius, int64_t* idxs,
                           float* dists, int32_t* counts, void* workspace, size_t workspace_bytes, int reuse,
                           void* stream);

/*
 * FEATURE MATCHING: the one or two nearest rows of a descriptor table for every row of another, and the filters that
 * make putative correspondences of them -- Open3D's correspondences_from_features(mutual_filter), PCL's correspondence
 * estimation with its rejectors -- device half of functions/match.py (csrc/feature_match.hip, feature_screen.h).
 *   f1 = p1 (N,P1,D), f2 = p2 (N,P2,D) fp32, 1 <= D < 2^16; lengths1, lengths2 (N,) int64.
 *   1. (d1, j1) and (d2, j2) are columns 0 and 1 of pointops_knn_points_idx(p1, p2, lengths1, lengths2, norm 2, K = 2):
 *      squared L2 as the unfused fp32 sum in d order, ties to the lower index.
 *   2. Row i HAS A NEAREST when i < lengths1[n] and lengths2[n] >= 1; it HAS A SECOND when also lengths2[n] >= 2.
 *   3. A row is KEPT when it has a nearest and passes every filter that is set:
 *        max_distance m  d1 < fl32(fl32(m) * fl32(m))   (ball query's comparison)
 *        ratio rho       d1 < fl32(fl32(rho) * fl32(rho)) * d2 with an fp32 product; rows without a second pass
 *        mutual          the K = 1 search of p2 over p1 returns i for row j1
 *   4. corr (N,P1) int64 = j1 where the row is kept, else -1 (what pointops_ransac_alignment takes);
 *      dists (N,P1) = d1 where the row has a nearest, else 0;  second (N,P1) = d2 where it has a second, +inf where it
 *      has a nearest only, 0 where it has none;  num_matches (N,) int64 = the rows with corr >= 0.
 *   Steps 3 and 4 are elementwise and live in functions/match.py; the entry below is step 1.
 *
 * pointops_feature_knn: idxs (N,P1,K) int64 and dists (N,P1,K) fp32 in pointops_knn_points_idx's conventions (0 for
 * rows >= lengths1[n] and slots >= lengths2[n]), byte-equal to that entry on the same inputs on every path; 1 <= K <= 2.
 *   Two paths.  The EXACT SEARCH is pointops_knn_points_idx itself (version -1).  The SCREEN orders the targets of a
 *   query by s = fl(fl(n1 + n2) - 2 g) -- norms and dot product as fmaf chains, the dot products on the matrix cores
 *   (v_mfma_f32_32x32x2_f32, queries on the column side: an accumulator lane owns one query and 16 targets of a 32 x 32
 *   block) -- keeps the 8 smallest (s, j) per lane, computes the exact distance of the 16 collected targets of a
 *   query and certifies the row when fl(r_K + E) < s_cut, E = (4 D + 8)(2^-24 (n1 + n2max) + 2^-149) rounded upwards
 *   (feature_screen.h has the definitions and the proof that then no dropped target can be among the K nearest, ties
 *   included).  Rows it cannot certify -- a near-tie across the cut, a norm that is not finite or above 2^126 -- go
 *   into a per-cloud device list and through the exact all-pairs kernel; that launch is always enqueued and ends on
 *   the device-side count.  Which path a row takes depends on the input alone and changes no byte; no float atomics,
 *   nothing read back, a fixed launch sequence: two calls are byte-equal and the call can be captured in a HIP graph.
 *   Dispatch: the screen takes 8 < D <= 128 where it was measured faster than the exact search (profiles/
 *   match_bench.jsonl): at least 65536 targets and at least 1024 workgroups of 128 queries; every other call is the
 *   exact search.  POINTOPS_DEBUG=match_screen=0|1 forces the exact search / the screen (any D <= 128).
 *   stats (N,4) int32, written by the call: 1 if the cloud went through the screen, its rows certified by the screen,
 *   its rows sent to the exact kernel, 0.
 *   workspace: pointops_feature_knn_workspace_bytes(N, P1, P2, D, K); a short or null one is POINTOPS_EWORKSPACE with
 *   nothing launched.  N, P1, P2 >= 0 below 2^31, 1 <= D < 2^16, K in {1, 2}, non-null pointers unless N or P1 is 0: anything
 *   else is POINTOPS_EINVAL.
 */
size_t pointops_feature_knn_workspace_bytes(int64_t N, int64_t P1, int64_t P2, int64_t D, int64_t K);
int pointops_feature_knn(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int64_t N,
                         int64_t P1, int64_t P2, int64_t D, int64_t K, int64_t* idxs, float* dists, int32_t* stats,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * Test support, as pointops_knn_grid_stats is: what the screen of pointops_feature_knn computes, from the same tile
 * code, for small shapes (P1, P2 <= 1024, D <= 128).  s (N,P1,P2): the screen value of every pair with
 * i < lengths1[n] and j < lengths2[n], 0 elsewhere;  n1 (N,P1), n2 (N,P2): the norms of every row;  n2max (N,): the
 * largest n2 over j < lengths2[n] (0 for none);  E (N,P1): the bound of every row i < lengths1[n] of a cloud with
 * lengths2[n] >= 1, 0 elsewhere.
 */
int pointops_feature_screen_values(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                                   int64_t N, int64_t P1, int64_t P2, int64_t D, float* s, float* n1, float* n2,
                                   float* n2max, float* E, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POINTOPS_AMD_H_ */
