/*
 * brd.h -- C ABI of the MI355X-native two-stage bidiagonal reduction
 * (libbrd_hip.so, built from svdsolver_amd/csrc/).
 *
 * Plain pointers and sizes; no exceptions, no C++ or torch types cross this
 * boundary.  Every entry point returns BRD_OK (0) or a negative brd_status;
 * brd_last_error() gives a human-readable message for the calling thread.
 *
 * Storage: row-major (the layout of csc586::gpu::Matrix<T>::flatten(),
 * matrix_gpu.h:223), element (i,j) at A[i*lda + j].
 *
 * Which reference interface each entry point replaces:
 *   brd_ge2band_*   csc586::gpu::cuda_brd_p1(Matrix<float>& A, size_t b)
 *                   (reference svd_cuda_2.cu:1117; svd_cuda_1.cu:750) and the
 *                   CPU csc586::parallel::brd_p1<T>(Matrix<T>&, size_t)
 *                   (svd_parallel.h:411).  Dense N x N -> upper band with b
 *                   super-diagonals, in place.  Unlike the reference GPU path
 *                   it is not fp32-only.
 *   brd_band2bd_*   csc586::parallel::brd_p2<T>(Matrix<T>&, size_t b)
 *                   (svd_parallel.h:640; twin gpu::brd_p2, svd_cpu.h:631) --
 *                   band -> bidiagonal, in place, returning d and e like the
 *                   reference's Bidiagonal{d, e} (svd_parallel.h:691).
 *   brd_dist_*,     new (the reference has no multi-GPU path):
 *   brd_ge2band_dist_*  block-cyclic column-sharded stage 1 over RCCL / xGMI.
 */
#ifndef BRD_H_
#define BRD_H_

#ifdef __cplusplus
extern "C" {
#endif

enum brd_status {
    BRD_OK = 0,
    BRD_EINVAL = -1,      /* bad argument (sizes, band width, null pointer)        */
    BRD_EHIP = -2,        /* HIP runtime error (message in brd_last_error)         */
    BRD_ENOMEM = -3,      /* device allocation failed                              */
    BRD_ERCCL = -4,       /* RCCL error                                            */
    BRD_EUNSUPPORTED = -5 /* valid request this build does not implement           */
};

/* flags */
#define BRD_DEVICE_PTR 0x1u   /* A, d, e are device pointers (else host; staged)   */
#define BRD_ASYNC      0x2u   /* device pointers only: return without syncing      */
#define BRD_COMPAT     0x0u   /* stage 2: the reference's window geometry (default)*/
#define BRD_EXACT_ORDER 0x4u  /* stage 2 compat, evaluated in the reference's exact
                                 operation order (bit-identical to the reference's
                                 CPU code; slow, for verification)                 */
#define BRD_NO_EXTRACT 0x8u   /* stage 2: do not write d/e (may pass NULL)         */
#define BRD_SIGMA      0x10u  /* stage 2: sigma-preserving geometry -- the reference's
                                 windows plus the final window pair each sweep
                                 needs, so the result is orthogonally equivalent
                                 to the band (not in the reference; combines
                                 with BRD_EXACT_ORDER)                            */

/* Stage 1: dense m x n (m >= n) -> upper band, bandwidth b (1 <= b <= 32).
 * On return A holds the band matrix: entries (i,j) with 0 <= j-i <= b, and
 * exact zeros elsewhere.  ngpus must be 1 (multi-GPU: brd_ge2band_dist_*). */
int brd_ge2band_f64(double *A, int m, int n, int lda, int b, int ngpus, unsigned flags);
int brd_ge2band_f32(float *A, int m, int n, int lda, int b, int ngpus, unsigned flags);

/* Stage 2: n x n band (bandwidth b) -> bidiagonal, in place, with the
 * reference's window geometry (BRD_COMPAT) or the sigma-preserving one
 * (BRD_SIGMA).  d (n) and e (n-1) receive the diagonal and super-diagonal
 * (same memory kind as A; e may be NULL when n = 1). */
int brd_band2bd_f64(double *A, int n, int lda, int b, double *d, double *e, unsigned flags);
int brd_band2bd_f32(float *A, int n, int lda, int b, float *d, float *e, unsigned flags);

/* Singular values of the upper bidiagonal (d (n), e (n-1)), host memory, in
 * descending order into sv (n): Golub-Kahan QR with Wilkinson shifts, values
 * only (replaces the reference's serial::qrd, svd_serial.h:368).  After
 * brd_band2bd_* with BRD_SIGMA these are the singular values of the matrix
 * stage 1 started from. */
int brd_bdsvd_f64(const double *d, const double *e, int n, double *sv);
int brd_bdsvd_f32(const float *d, const float *e, int n, float *sv);

/* The same on the GPU: d (n), e (n-1) and sv (n) are DEVICE pointers; the
 * values (descending) are bracketed by multisection on the Golub-Kahan
 * tridiagonal (every value independently, G lanes each), to the host QR's
 * accuracy (|sigma_i - exact| ~ eps sigma_max).  Runs on the library stream;
 * BRD_ASYNC returns without waiting.  e may be NULL when n = 1. */
int brd_bdsvd_dev_f64(const double *d, const double *e, int n, double *sv, unsigned flags);
int brd_bdsvd_dev_f32(const float *d, const float *e, int n, float *sv, unsigned flags);

/* SVD of `batch` small m x n matrices (n <= m; n <= 64, m <= 128), one launch:
 * A_i = U_i diag(S_i) V_i^T by one-sided Jacobi.  All pointers are DEVICE
 * pointers; matrices are row-major: A_i = A + i*stride_a, element (r,c) at
 * [r*lda + c].  S: batch x n, descending, S_i = S + i*n.  U (m x n per matrix)
 * and V (n x n per matrix: V, not V^T) may both be NULL: values only.
 * info: batch ints, required (0 converged, 1 sweep cap, 2 non-finite input).
 * A is not modified.  Runs on the library stream; BRD_ASYNC returns without
 * waiting.  Sizes beyond the limits: BRD_EUNSUPPORTED. */
int brd_svd_batched_f64(const double *A, int batch, int m, int n, int lda, long stride_a,
                        double *S, double *U, int ldu, long stride_u,
                        double *V, int ldv, long stride_v, int *info, unsigned flags);
int brd_svd_batched_f32(const float *A, int batch, int m, int n, int lda, long stride_a,
                        float *S, float *U, int ldu, long stride_u,
                        float *V, int ldv, long stride_v, int *info, unsigned flags);

/* The same for mid-size matrices: 1 <= n <= m <= 128 (beyond 128 x 128:
 * BRD_EUNSUPPORTED), one launch, one workgroup per matrix.  Arguments, layout,
 * outputs, info, the NULL rules for U and V and flags are exactly those of
 * brd_svd_batched_*; no workspace and no per-stream state, A is not modified.
 * n <= 64 forwards to brd_svd_batched_* (bitwise its result).  For n > 64 in
 * fp64 with vectors the kernel keeps its working copy of V in the caller's V
 * block (only the n x n entries are ever touched), so V holds the result only
 * when the call's work on the stream is done, like every other output. */
int brd_svd_mid_batched_f64(const double *A, int batch, int m, int n, int lda, long stride_a,
                            double *S, double *U, int ldu, long stride_u,
                            double *V, int ldv, long stride_v, int *info, unsigned flags);
int brd_svd_mid_batched_f32(const float *A, int batch, int m, int n, int lda, long stride_a,
                            float *S, float *U, int ldu, long stride_u,
                            float *V, int ldv, long stride_v, int *info, unsigned flags);

/* Batched SVD of tall matrices: any m >= n with 1 <= n <= 64 (n > 64:
 * BRD_EUNSUPPORTED).  Householder QR of every matrix in row blocks (A = Q R,
 * A read once), brd_svd_batched's Jacobi kernel on the n x n factors R, then
 * U = Q U_R: three launches on the library stream with no host
 * synchronisation between them.  Arguments, layout, outputs, info and flags
 * are exactly those of brd_svd_batched_*; column scaling keeps the relative
 * accuracy (QR does not mix columns).  m <= 128 forwards to brd_svd_batched_*
 * (bitwise its result; needs no workspace).
 * work: device memory of at least brd_svd_tall_batched_work_bytes(batch, m, n,
 * vectors, elem_bytes) bytes (vectors: 1 when U and V are given, else 0;
 * elem_bytes: 8 or 4), owned by the caller and free again when the call's
 * work on the stream is done; it holds R and, with vectors, U_R and one
 * Householder scalar per column per row block.  The query returns a negative
 * brd_status for sizes the call rejects and 0 when nothing is needed (work
 * may then be NULL); work_bytes too small: BRD_EINVAL. */
long brd_svd_tall_batched_work_bytes(int batch, int m, int n, int vectors, int elem_bytes);
int brd_svd_tall_batched_f64(const double *A, int batch, int m, int n, int lda, long stride_a,
                             double *S, double *U, int ldu, long stride_u,
                             double *V, int ldv, long stride_v, int *info,
                             void *work, long work_bytes, unsigned flags);
int brd_svd_tall_batched_f32(const float *A, int batch, int m, int n, int lda, long stride_a,
                             float *S, float *U, int ldu, long stride_u,
                             float *V, int ldv, long stride_v, int *info,
                             void *work, long work_bytes, unsigned flags);

/* Batched SVD behind one entry point: any m >= n with 1 <= n <= 128 (n > 128:
 * BRD_EUNSUPPORTED).  Arguments, layout, outputs, info, the NULL rule for U
 * and V, flags, the argument checks and their order are those of
 * brd_svd_tall_batched_*.  The call picks the route by size:
 *   m <= 128, n <= 64: brd_svd_batched_*'s launch (bitwise its result);
 *   m <= 128, n >  64: brd_svd_mid_batched_*'s launch (bitwise its result);
 *   m >  128, n <= 64: brd_svd_tall_batched_*'s three launches (bitwise);
 *   m >  128, n >  64: Householder QR in row blocks of 128 rows (A read once),
 *     brd_svd_mid_batched's Jacobi kernel on the n x n factors R, U = Q U_R;
 *     three launches with no host synchronisation between them.  In fp64 with
 *     vectors the Jacobi step keeps its working V in the caller's V block, as
 *     for brd_svd_mid_batched_*.
 * work: as for brd_svd_tall_batched_*, of at least
 * brd_gesvd_batched_work_bytes(batch, m, n, vectors, elem_bytes) bytes: 0 when
 * m <= 128, brd_svd_tall_batched_work_bytes for n <= 64, and for n > 64
 * batch * (n^2 + vectors * (n^2 + ceil(m / 128) * n)) * elem_bytes: R, U_R and
 * one Householder scalar per column per row block.  On that last route R's
 * upper triangle and U_R are also the kernels' working storage. */
long brd_gesvd_batched_work_bytes(int batch, int m, int n, int vectors, int elem_bytes);
int brd_gesvd_batched_f64(const double *A, int batch, int m, int n, int lda, long stride_a,
                          double *S, double *U, int ldu, long stride_u,
                          double *V, int ldv, long stride_v, int *info,
                          void *work, long work_bytes, unsigned flags);
int brd_gesvd_batched_f32(const float *A, int batch, int m, int n, int lda, long stride_a,
                          float *S, float *U, int ldu, long stride_u,
                          float *V, int ldv, long stride_v, int *info,
                          void *work, long work_bytes, unsigned flags);

/* Batched least squares and pseudo-inverse through the batched SVD: for every
 * matrix, the minimum-norm x minimising |A x - b|_2,
 *     X = V diag(sigma+) U^T B,   sigma+_j = 1 / sigma_j where sigma_j > rcond sigma_1, else 0,
 * from brd_gesvd_batched_*'s factors (its launches, then one more, on the
 * library stream with no host synchronisation between them).  Shapes are those
 * of brd_gesvd_batched_*: m >= n, 1 <= n <= 128 (n > 128: BRD_EUNSUPPORTED),
 * any m; all pointers are DEVICE pointers, everything is row-major.
 *   B: m x nrhs per matrix (element (r,c) of matrix i at B[i*stride_b + r*ldb + c]),
 *   X: n x nrhs per matrix, likewise with ldx, stride_x.
 * BRD_LS_TRANS solves A^T x = b instead (the minimum-norm solution; how wide
 * problems are posed): B is then n x nrhs and X is m x nrhs.
 * B == NULL stands for the identity and nrhs is ignored: X is n x m, the
 * pseudo-inverse of A (with BRD_LS_TRANS m x n, the pseudo-inverse of A^T).
 * rcond < 0 selects max(m, n) * eps of the type.  S (batch x n, the singular
 * values, descending) and rank (batch ints: the number of values kept) may be
 * NULL.  info: batch ints, required, as for brd_gesvd_batched_*; a matrix with
 * info 2 (non-finite A) gets NaN in X and rank -1.  A and B are not modified;
 * X must not overlap them.  BRD_ASYNC returns without waiting.
 * work: device memory, 256-byte aligned, of at least
 * brd_gelss_batched_work_bytes(batch, m, n, nrhs, elem_bytes) =
 *   r(brd_gesvd_batched_work_bytes(batch, m, n, 1, elem_bytes))
 *   + r(batch m n elem_bytes) + r(batch n n elem_bytes) + r(batch n elem_bytes)
 * bytes with r(x) = x rounded up to a multiple of 256: brd_gesvd_batched's own
 * workspace, U, V and S in this order (nrhs does not enter: the solve keeps
 * its working tile on chip).  The query returns a negative brd_status for
 * sizes the call rejects.
 * Argument checks: those of brd_gesvd_batched_* first, in its order; then
 * nrhs >= 1 (B given), ldb / stride_b, ldx / stride_x, X non-NULL, work. */
#define BRD_LS_TRANS 0x20u   /* solve A^T x = b (minimum norm): B is n x nrhs, X is m x nrhs */
long brd_gelss_batched_work_bytes(int batch, int m, int n, int nrhs, int elem_bytes);
int brd_gelss_batched_f64(const double *A, int batch, int m, int n, int lda, long stride_a,
                          const double *B, int nrhs, int ldb, long stride_b,
                          double *X, int ldx, long stride_x,
                          double rcond, double *S, int *rank, int *info,
                          void *work, long work_bytes, unsigned flags);
int brd_gelss_batched_f32(const float *A, int batch, int m, int n, int lda, long stride_a,
                          const float *B, int nrhs, int ldb, long stride_b,
                          float *X, int ldx, long stride_x,
                          float rcond, float *S, int *rank, int *info,
                          void *work, long work_bytes, unsigned flags);

/* Stream used by subsequent calls (hipStream_t; NULL = the legacy default
 * stream).  Until the first call the library uses a stream of its own;
 * brd_use_own_stream() reverts to it. */
int brd_set_stream(void *hip_stream);
int brd_use_own_stream(void);

/* Two reductions side by side (a stream of matrices): stage 2 of matrix i on
 * one stream while stage 1 of matrix i+1 runs on another.  s2_cus > 0 runs
 * every stage-2 sweep on that many workgroups (one per CU; the bundle chain
 * keeps fewer than ~64 busy at N <= 16384) and sizes stage-1 launches for the
 * remaining CUs; 0 restores the defaults (each stage on the whole chip).
 * No reference counterpart (the reference runs one reduction at a time,
 * svd_cuda_2.cu:1387 / timing.h:55). */
int brd_set_overlap(int s2_cus);   /* 0 <= s2_cus < device CUs, else BRD_EINVAL */

/* Drains every stream the library has launched on and reports failures of
 * asynchronous (BRD_ASYNC) calls: a stage-2 sweep whose bounded spin gave up
 * (its output is then invalid) or a pending HIP error.  The stage-2 error
 * word of a stream is sticky: no launch resets it; a synchronous band2bd on
 * that stream or this call reads and clears it.  Call it after a batch of
 * asynchronous work before trusting the results. */
int brd_check_errors(void);

/* Drain hip_stream (NULL: the library's current stream) and free the
 * library's per-stream state for it: stage-1/stage-2 workspaces, the cached
 * HBM staging buffer of host-pointer calls, the stage-2 error word (read
 * first: BRD_EHIP if it was set).  brd_check_errors() visits every stream the
 * library has launched on, so call this before destroying such a stream.
 * Host-pointer calls keep their staging buffer until then (with
 * BRD_STAGE_KEEP_MB set, one larger than that many MiB is freed on return). */
int brd_release_stream(void *hip_stream);

/* Per-kernel device timing for roofline reporting.  While enabled, the library
 * brackets every launch of the named kernel class with HIP events on the
 * launch stream.  kernel: "s1_apply", "s1_factor", "s2_sweep", "svd_batched"
 * (credited with the bytes of A read and of S, U, V, info written; no flops:
 * the sweep count depends on the data), "svd_mid_batched" (one entry per
 * brd_svd_mid_batched_* call, forwarded calls included, credited like
 * "svd_batched"), "svd_tall_batched" (one entry per
 * call spanning its three launches, credited like "svd_batched"; the stages
 * of a call beyond 128 rows also under "svd_tall_qr", "svd_tall_jacobi" and
 * "svd_tall_apply", time only), "gesvd_batched" (one entry per
 * brd_gesvd_batched_* call on any route, credited like "svd_batched"; such a
 * call records nothing under the three kinds before, and the stages of its
 * two routes beyond 128 rows also under "svd_tall_qr", "svd_tall_jacobi" and
 * "svd_tall_apply", time only), "gelss_batched" (one entry per
 * brd_gelss_batched_* call, credited with the bytes of A and B read and of X
 * and S written; such a call records nothing under "gesvd_batched" or the
 * kinds before it, its SVD stages beyond 128 rows under the three
 * "svd_tall_*" kinds and its last launch under "gelss_solve", time only).
 * Returns the
 * number of launches, their total device time in ms and the algorithmic flops
 * and bytes those launches were credited with. */
int brd_profile_enable(int enable);
int brd_profile_reset(void);
int brd_profile_query(const char *kernel, long long *launches, double *total_ms,
                      double *flops, double *bytes);

/* ---- Multi-GPU stage 1 (one process per GPU) ------------------------------
 * Layout: 1-D block-cyclic over column panels of width b -- global panel p
 * (columns [p b, p b + b)) lives on rank p mod P as local panel p / P.  A
 * rank's shard is m x n_loc (n_loc = brd_dist_local_cols), row-major with
 * leading dimension lda_loc, in device memory.  The stage-2 input is
 * assembled on one rank with brd_dist_gather_band.
 * Collectives go to RCCL over xGMI (brd_dist_init, with an id from
 * brd_dist_unique_id on one rank, shared out of band) or to a host callback
 * (brd_dist_init_host: the library drains its stream, then calls fn, which
 * must complete the collective on the device buffers before returning).
 * A communicator belongs to the library stream current at its init
 * (brd_set_stream); the first one is also the default for streams without
 * their own.  Calls on a stream use that stream's communicator and a
 * workspace of that stream, so several matrices' distributed reductions can
 * run at once, one stream (and communicator) each; every rank must issue a
 * communicator's calls in the same order.  brd_dist_finalize releases all. */
enum brd_coll_op {
    BRD_COLL_BCAST = 0,         /* recv (== send) broadcast from root, count elems */
    BRD_COLL_ALLGATHER = 1,     /* send: count elems; recv: count * nranks elems    */
    BRD_COLL_ALLREDUCE_SUM = 2  /* in place (send == recv), count elems             */
};
enum brd_dtype { BRD_DT_BYTE = 0, BRD_DT_F32 = 1, BRD_DT_F64 = 2 };
typedef int (*brd_coll_fn)(int op, const void *send, void *recv, unsigned long count, int dtype, int root,
                           void *user);

int brd_dist_unique_id(void *id_out, int id_bytes);      /* id_bytes >= 128 */
int brd_dist_init(int rank, int nranks, const void *id, int id_bytes);
int brd_dist_init_host(int rank, int nranks, brd_coll_fn fn, void *user);
int brd_dist_finalize(void);
int brd_dist_local_cols(int n, int b, int nranks, int rank);   /* n_loc of a rank (>= 0) */
/* Stage 1 on the sharded matrix (every rank calls; BRD_DEVICE_PTR required). */
int brd_ge2band_dist_f64(double *A_loc, int m, int n, int lda_loc, int b, unsigned flags);
int brd_ge2band_dist_f32(float *A_loc, int m, int n, int lda_loc, int b, unsigned flags);
/* Assemble the band (diagonals 0..b) on rank root into the dense m x n matrix
 * B (device, ldb >= n; zero outside the band).  B is ignored on other ranks. */
int brd_dist_gather_band_f64(const double *A_loc, int m, int n, int lda_loc, int b, double *B, int ldb, int root,
                             unsigned flags);
int brd_dist_gather_band_f32(const float *A_loc, int m, int n, int lda_loc, int b, float *B, int ldb, int root,
                             unsigned flags);

const char *brd_last_error(void);
int brd_version(void);

#ifdef __cplusplus
}
#endif

#endif /* BRD_H_ */
