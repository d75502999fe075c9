/*
 * rsvd_c.h -- C ABI of the MI355X-native randomized-SVD engine (librsvd_hip.so).
 *
 * Plain pointers and sizes only: no torch, Eigen or HIP types cross this boundary (streams are
 * passed as `void*` = hipStream_t).  Every entry point returns an rsvd_status_t and never throws.
 *
 * Boundary mapping (reference = AMSC22-23/rSVD_Kamaneh_Raganato_Terrana @ 2024-10-08):
 *   rsvd_run / rsvd_run_host_f64    <- void rSVD(Mat_m& A, Mat_m& U, Vec_v& S, Mat_m& V, int l,
 *                                          SVDMethod)             include/rSVD.hpp:14, src/rSVD.cpp:72-133
 *   rsvd_range_finder              <- void intermediate_step(const Mat_m& A, Mat_m& Q,
 *                                          const Mat_m& Omega, int l, int q)
 *                                                                  include/rSVD.hpp:13, src/rSVD.cpp:57-70
 *   rsvd_generate_omega            <- Mat_m generateOmega(int n, int l)
 *                                                                  include/rSVD.hpp:15, src/rSVD.cpp:12-55
 *   rsvd_qr (full = 0 / 1)         <- void qr_decomposition_reduced/full(const Mat_m& A, Mat_m& Q,
 *                                          Mat_m& R)              include/QR.hpp:15-16, src/QR.cpp:22-80
 *   rsvd_svd                       <- template<SVDMethod> SVD::compute()/getU/getS/getV
 *                                                                  include/SVD_class.hpp:35-71,79-180
 *   rsvd_run_batched               <- one rSVD per block, Image::compress_parallel
 *                                                                  image_compression/src/image_com.cpp:350-371
 *   rsvd_compress_batched /        <- localMatrix = U * S.asDiagonal() * V.transpose() put back into the
 *   rsvd_lowrank /                    image (image_com.cpp:374, :381-394; Image::reconstruct :184-190) and
 *   rsvd_compress_host_f64            ||A - U diag(S) V^T||_F (tests/rSVD_test.cpp:77-95)
 *   rsvd_pod / rsvd_pod_host_f64   <- class POD: standard_POD / energy_POD / weight_POD, ns <= Nh branch
 *                                     POD/ParametricDiffusion1D/src/POD.{hpp,cpp} (:136-224, :227-336, :339-462)
 * The C++ drop-in headers include/rSVD.hpp, include/QR.hpp, include/SVD_class.hpp, include/POD.hpp sit on top of
 * these symbols with the reference's exact signatures.
 *
 * Layouts: every matrix is COLUMN-major (Eigen's default) with an explicit leading dimension.
 * Device-pointer entry points are asynchronous on the handle's stream; *_host_* variants copy
 * host buffers in and out and synchronise.
 */
#ifndef RSVD_C_H
#define RSVD_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSVD_ABI_VERSION 9

typedef enum {
    RSVD_OK = 0,
    RSVD_ERR_INVALID_ARG = 1,    /* bad sizes / pointers (Eigen would assert)                      */
    RSVD_ERR_UNSUPPORTED = 2,    /* e.g. SVD method not available; maps to std::invalid_argument     */
    RSVD_ERR_HIP = 3,            /* a HIP runtime / launch error (see rsvd_last_error)              */
    RSVD_ERR_NO_DEVICE = 4,
    RSVD_ERR_NUMERICAL = 5,      /* non-finite result                                              */
    RSVD_ERR_COMM = 6            /* the distributed all-reduce callback failed                      */
} rsvd_status_t;

/* Storage / compute type of A.  F64: fp64 end to end (the reference's arithmetic class).
 * F32: fp32 MFMA projections and fp32 panels; Grams accumulated in fp64 (f64 MFMA), the panel
 * products by R^-1 in fp64, Cholesky factor and small Jacobi SVD in fp32.
 * BF16 / FP8_E4M3 (OCP e4m3fn): A stored in that type (A = a_scale * stored value), projections
 * on the bf16 MFMA with a hi/lo-split fp32 skinny operand, fp32 panels, fp64 Grams / Cholesky /
 * small SVD; Omega is the Philox Gaussian rounded to bf16 (resp. e4m3); U, S, V, Omega and Q are
 * fp32 at the ABI. */
typedef enum { RSVD_F64 = 0, RSVD_F32 = 1, RSVD_BF16 = 2, RSVD_FP8_E4M3 = 3 } rsvd_dtype_t;

/* Dynamic range.  The reference computes in fp64 Eigen on data in physical units, and its results
 * are equivariant under scaling: A 2^k has the singular values of A times 2^k and its singular
 * vectors.  Guaranteed here, for every entry point and dtype: scaling A by 2^k, or passing
 * a_scale = 2^k, scales S by 2^k and leaves U, V, the Q of rsvd_range_finder and the Q of rsvd_qr
 * unchanged within the parity bounds of that dtype; R of rsvd_qr and C of rsvd_compress_batched /
 * rsvd_lowrank scale by 2^k and their err2 by 2^(2k) (err2[0], a sum of exactly widened squares in
 * a fixed order, exactly); rsvd_pod's C and sigma scale by 2^(2k) and, without the textbook flag,
 * W by 2^-k.  This holds for sigma_max(A) up to the test matrices' (at most 16.3) and
 *   |k| <= 40    where results are delivered in fp32 (F32, BF16, FP8_E4M3 A): the squares of all
 *                singular values, and sums of 2^20 of them, are ordinary fp32 numbers there;
 *   |k| <= 240   for F64 A.
 * (tests/test_gpu_scale.py; the measured errors are tabulated in DESIGN.md §4.1.)
 * Outside the window: where the small SVD is the one-workgroup Jacobi (rsvd_run with l <= 64 on
 * F64 / F32 A, BF16 / FP8_E4M3 A at l <= 64, rsvd_svd's Jacobi at min(m, n) <= 64) and in the fused
 * kernel of rsvd_run_batched / rsvd_compress_batched, a run either still meets those bounds or ends
 * in RSVD_ERR_NUMERICAL through rsvd_sync (for a batched call also bit 1 of the matrix's info
 * word), never in RSVD_OK with wrong numbers: a W = (Q^T A) whose largest entry lies outside
 * 2^+-56 (fp32 Jacobi: F32 A, and the fp32 batched kernel) or 2^+-480 (fp64 Jacobi) is reported in
 * that way (tested at 2^+-100 for an F32 rsvd_run and an fp32 batch).  The other paths (the wide
 * engines' eigensolver and block Jacobi, rsvd_qr, rsvd_lowrank, rsvd_pod) carry no such check and
 * have not been run outside the window: there only non-finite S is reported.
 * Not equivariant, as in the reference, whose stop rules there are absolute: RSVD_SVD_POWER and
 * RSVD_SVD_POWER_IC ("sigma < 1e-12"), RSVD_SVD_PARALLEL_JACOBI of rsvd_svd (pair weight
 * max(1e-12, 1e-12 maxDiag), deno < 1e-10) and rsvd_pod's svd_type 2 where it follows that path. */

/* Mirrors enum class SVDMethod { Jacobi, Power, ParallelJacobi } (include/SVD_class.hpp:28-32).
 * RSVD_SVD_POWER_IC (rsvd_run / rsvd_range_finder only) is image_compression's power-method small
 * SVD behind its 5-argument rSVD (image_compression/src/SVD.cpp:30-55, PowerMethod.cpp:3-43): B is
 * recomputed as A^T A of the deflated matrix after every triplet and there is no sigma < 1e-12 stop
 * (a triplet with sigma == 0, where the reference divides by zero, ends it); V in columns. */
typedef enum {
    RSVD_SVD_JACOBI = 0,
    RSVD_SVD_POWER = 1,
    RSVD_SVD_PARALLEL_JACOBI = 2,
    RSVD_SVD_POWER_IC = 3
} rsvd_svd_method_t;

/* Orthonormalisation of the tall-skinny panels.  AUTO = CholeskyQR (one pass for fp32 power-
 * iteration intermediates, two otherwise) with a predicated Gram-Schmidt (CGS2) re-
 * orthonormalisation of the panel when a Cholesky pivot breaks down (rank-deficient or too
 * ill-conditioned sketch).  GS2 = always the CGS2 path (single-GPU panels).
 * CHOLQR2 = two CholeskyQR passes on every panel. */
typedef enum { RSVD_QR_AUTO = 0, RSVD_QR_GS2 = 1, RSVD_QR_CHOLQR2 = 2 } rsvd_qr_mode_t;

/* rsvd_desc_t.flags.  LOWP_INTERMEDIATES (bf16 / e4m3 A, q >= 2): the two projections of power
 * iterations 1 .. q-1 take the fp32 skinny operand as its bf16 rounding alone (one MFMA pass
 * instead of the hi + lo pair); the last iteration, B^T = A^T Q and the outputs keep 16-bit
 * operands.  An error injected there is damped by the later iterations by about
 * (sigma_{l+1} / sigma_{l/2})^2 each: on spectra that decay across the sketch (e.g. 0.985^i at
 * l = 256) the results stay within 1e-5 of the full-precision path, on flat ones (0.999^i) they
 * drift to ~5e-3.  Off by default. */
#define RSVD_FLAG_LOWP_INTERMEDIATES 1
/* Test/diagnostic flag (ABI 6): run the n-side sharded code path (reduce-scatter / all-gather
 * through the handle's collectives) even at world 1, so a one-GPU box exercises the exact RCCL
 * calls an N-GPU run makes.  Requires collectives (rsvd_set_collectives or rsvd_comm_init). */
#define RSVD_FLAG_FORCE_NSHARD 2

typedef struct {
    int64_t m, n;              /* A is m x n                                                   */
    int64_t lda;               /* >= m                                                         */
    int32_t l;                 /* sketch width k + p (the reference's `l`)                     */
    int32_t q;                 /* power iterations; the reference hard-codes 2 (src/rSVD.cpp:83) */
    int32_t dtype;             /* rsvd_dtype_t                                                 */
    int32_t method;            /* rsvd_svd_method_t                                            */
    int32_t qr_mode;           /* rsvd_qr_mode_t                                               */
    int32_t flags;             /* RSVD_FLAG_* (ABI 5; the former reserved word, 0 = defaults)  */
    uint64_t seed;             /* Philox key for Omega when no Omega is supplied               */
    double a_scale;            /* A = a_scale * (stored A); 0 means 1 (any dtype; S scales by
                                  |a_scale|, V flips sign when a_scale < 0)                        */
} rsvd_desc_t;

/* Diagnostics of the last run on a handle. */
typedef struct {
    int32_t cholqr_fallbacks;  /* panels re-orthonormalised by the CGS2 fallback                 */
    int32_t jacobi_sweeps;     /* sweeps of the small SVD                                      */
    int32_t splits_nn, splits_tn; /* K splits chosen for the projections                         */
    int32_t power_kept;        /* SVDMethod::Power: triplets found before sigma < 1e-12 (else 0)  */
    int32_t n_shard_rows;      /* n-side rows per rank of a sharded n side (ABI 5), 0: replicated */
} rsvd_info_t;

typedef struct rsvd_handle_s *rsvd_handle_t;

/* Distributed exchange hook: sum `count` elements of `dtype` at device pointer `buf` over all
 * ranks, in place, ordered after the work already enqueued on `stream`.  Return 0 on success.
 * (The Python front end binds it to torch.distributed.all_reduce over RCCL.) */
typedef int (*rsvd_allreduce_fn)(void *buf, int64_t count, int32_t dtype, void *stream, void *user);

/* Collective hook of the n-side sharding (ABI 5).  op RSVD_COLL_REDUCE_SCATTER: `send` holds
 * world x count elements, rank r receives the sum over ranks of elements [r count, (r + 1) count)
 * in `recv` (recv may alias send + rank count, in place).  op RSVD_COLL_ALL_GATHER: every rank
 * contributes `count` elements at `send` and receives all world x count, rank r's at
 * recv + r count (send may alias recv + rank count).  dtype: RSVD_F64, RSVD_F32 or RSVD_BF16.
 * Ordered after the work enqueued on `stream`; return 0 on success.  (The Python front end binds
 * it to torch.distributed.reduce_scatter_tensor / all_gather_into_tensor over RCCL.) */
typedef int (*rsvd_collective_fn)(int32_t op, void *send, void *recv, int64_t count, int32_t dtype, void *stream,
                                  void *user);
#define RSVD_COLL_REDUCE_SCATTER 1
#define RSVD_COLL_ALL_GATHER 2

const char *rsvd_status_string(int status);
int rsvd_abi_version(void);

int rsvd_create(int device, rsvd_handle_t *out);
int rsvd_destroy(rsvd_handle_t h);
int rsvd_set_stream(rsvd_handle_t h, void *hip_stream);
const char *rsvd_last_error(rsvd_handle_t h);
/* Synchronise the handle's stream and report what the queued runs could not report at enqueue
 * time: RSVD_ERR_HIP for an in-kernel hand-off or grid barrier that timed out,
 * RSVD_ERR_NUMERICAL for a rank-deficient panel the repair pass could not complete or for
 * non-finite singular values.  These conditions are sticky on the handle until reported (by this
 * call or rsvd_get_info), so one rsvd_sync after several asynchronous rsvd_run calls checks them
 * all.  The *_host_* entry points end with it. */
int rsvd_sync(rsvd_handle_t h);
/* rsvd_sync, then the diagnostics of the last run. */
int rsvd_get_info(rsvd_handle_t h, rsvd_info_t *info);
/* Row-sharded runs: this handle owns rows [offset, offset + m_local) of a global m x n A; the
 * hook sums the n x l partial products A_g^T Q_g and the l x l Grams across ranks. */
int rsvd_set_comm(rsvd_handle_t h, int rank, int world, rsvd_allreduce_fn fn, void *user);
/* Optional (ABI 5), after rsvd_set_comm: with a collective hook the wide engine (bf16 / e4m3 A,
 * or l > 64) also shards the n side -- rank r owns rows [r c, (r + 1) c) of the
 * n x l panels, c = n / world rounded up to 32: A^T Q is reduce-scattered instead of all-reduced,
 * each rank orthonormalises its rows (CholeskyQR with the l x l Gram all-reduced), the next
 * skinny operand and the final V are all-gathered.  fn = NULL switches back to the replicated
 * n side.  SVDMethod::Power runs keep the replicated n side.  rsvd_workspace_bytes covers the
 * padded n-side panels of any world up to 64; past 64 ranks the n side stays replicated. */
int rsvd_set_collectives(rsvd_handle_t h, rsvd_collective_fn fn, void *user);

/* Library-owned RCCL (ABI 6): the handle creates and owns an RCCL communicator over the ranks'
 * GPUs (one process per GPU, as the reference's MPI ranks, src/rSVD.cpp:15,20-23) and issues
 * ncclAllReduce / ncclReduceScatter / ncclAllGather on its own stream -- no hooks, no Python.
 * rsvd_comm_unique_id fills RSVD_COMM_ID_BYTES bytes (ncclGetUniqueId) on ONE rank; the caller
 * broadcasts them (e.g. MPI_Bcast, where the reference Bcasts Omega, src/rSVD.cpp:52) and every
 * rank calls rsvd_comm_init with its rank.  shard_n != 0 also shards the n side (as
 * rsvd_set_collectives).  rsvd_set_comm / rsvd_set_collectives afterwards replace it;
 * rsvd_comm_destroy (or rsvd_destroy) releases it.  librccl is loaded on first use
 * (RSVD_ERR_UNSUPPORTED when it cannot be). */
#define RSVD_COMM_ID_BYTES 128
int rsvd_comm_unique_id(void *id);
int rsvd_comm_init(rsvd_handle_t h, const void *id, int rank, int world, int shard_n);
int rsvd_comm_destroy(rsvd_handle_t h);

/* Row partition of src/rSVD.cpp:20-23 / src/PM.cpp:31-35: rows of rank `rank` out of `world`.
 * Host-only arithmetic (no device needed).  Returns the local row count, *offset = first row. */
int64_t rsvd_row_partition(int64_t rows, int world, int rank, int64_t *offset);

/* Device workspace bytes rsvd_run needs for `desc` (allocated lazily by the handle). */
int rsvd_workspace_bytes(const rsvd_desc_t *desc, size_t *bytes);
/* Timing mode (benchmarking): hipEvent pairs bracket every projection GEMM kernel launch
 * (A*X and A^T*Q; not their slab reductions).  rsvd_set_timing resets the accumulators;
 * rsvd_get_timing synchronises the stream and returns totals since the reset. */
typedef struct {
    int32_t nn_launches, tn_launches;
    double nn_ms, tn_ms;
    int32_t sketch_launches, reserved; /* the sketch Y = A Omega alone (also counted in nn_*): e4m3 A runs
                                          it on the fp8 MFMA, every other product on the bf16 / fp32 one */
    double sketch_ms;
} rsvd_timing_t;
int rsvd_set_timing(rsvd_handle_t h, int enable);
int rsvd_get_timing(rsvd_handle_t h, rsvd_timing_t *t);
/* Use caller-owned device memory as the workspace (NULL reverts to handle-owned memory).
 * The workspace's contents are unspecified on entry and on return: every run initialises what it
 * reads, no state is carried in the workspace between runs, and results do not depend on what it
 * held before (tests/test_gpu_workspace.py runs every engine over 0x00 / 0xFF / 0x4B fills). */
int rsvd_set_workspace(rsvd_handle_t h, void *ptr, size_t bytes);

/* ---- device-pointer entry points (asynchronous on the handle stream) ---------------------- */

/* rSVD: U (m x d, ldu), S (d), V (n x d, ldv), d = min(l, n); element type = desc->dtype (fp32
 * for BF16 / FP8_E4M3).  method POWER (src/rSVD.cpp:106-113): the reference's power method with
 * deflation on B = Q^T A (start vectors: Philox stream (seed ^ 0x504F574552) + i, the reference's
 * s(n) iterations); V's columns are the right singular vectors (the reference returns them as the
 * rows of an n x n V_ -- include/SVD_class.hpp rebuilds that layout); triplets past an early stop
 * (sigma < 1e-12) are zero and rsvd_get_info reports how many were kept.  omega: optional n x l column-major (ld = ldo) sketch in that element
 * type (rounded to bf16 / e4m3 for the low-precision types); NULL => Philox(desc->seed).
 * l <= 512 on the wide engine; 512 < l <= 4096 (the reference has no cap, src/rSVD.cpp:72) on one GPU
 * through dense_big.cpp's column-major blocks (MFMA GEMM products, block CGS2 + CholeskyQR3, the
 * block Jacobi small SVD -- or, for Power, the power method in the coordinates of Q_B on a persistent
 * grid; bf16 / e4m3 A widened to fp32 once), also row-sharded (RSVD_ERR_UNSUPPORTED for
 * RSVD_SVD_POWER_IC and past 4096). */
int rsvd_run(rsvd_handle_t h, const rsvd_desc_t *desc, const void *A, const void *omega, int64_t ldo,
             void *U, int64_t ldu, void *S, void *V, int64_t ldv);

/* intermediate_step: Q (m x l, ldq) orthonormal basis of the range of (A A^T)^q A Omega. */
int rsvd_range_finder(rsvd_handle_t h, const rsvd_desc_t *desc, const void *A, const void *omega, int64_t ldo,
                      void *Q, int64_t ldq);

/* generateOmega: n x l N(0,1), column-major (ld = n), element (i,j) = Philox stream element i+n*j.
 * dtype BF16 / FP8_E4M3: the same values rounded to bf16 / e4m3 (round half to even; e4m3
 * saturates at +-448), written as fp32 -- the Omega the low-precision rsvd_run draws. */
int rsvd_generate_omega(rsvd_handle_t h, int64_t n, int32_t l, uint64_t seed, int32_t dtype, void *omega);

/* QR() boundary <- qr_decomposition_reduced / qr_decomposition_full (include/QR.hpp:15-16,
 * src/QR.cpp:22-80).  full = 0: Q m x n (ldq), R n x n (ldr), requires m >= n (src/QR.cpp:78);
 * full = 1: Q m x m, R m x n (upper trapezoidal).  dtype F64 / F32.  Q has orthonormal columns
 * and A = Q R; R(j,j) >= 0 except on the leading columns of A whose sub-diagonal is already zero,
 * where R(j,j) = A(j,j) as the Givens sweep leaves them.  For full-rank A this is the unique QR,
 * i.e. the reference's; the complement Q[:, n:] of a full QR is an orthonormal completion
 * (identity columns for an A with trailing zero rows).  Up to 512 columns (of A, or of Q for the
 * full form) one shifted-CholeskyQR3 pass; past that, 512-column blocks by block CGS2 + CholeskyQR3
 * (dense_big.cpp), bounded only by device memory. */
int rsvd_qr(rsvd_handle_t h, int64_t m, int64_t n, const void *A, int64_t lda, int32_t dtype, int32_t full, void *Q,
            int64_t ldq, void *R, int64_t ldr);

/* SVD<method>::compute() boundary (include/SVD_class.hpp:35-97).  Jacobi / ParallelJacobi
 * (:100-180, :223-333): U m x k (ldu), S k (descending, >= 0), V n x k (ldv), k = min(m, n)
 * <= 4096 (past 512: block Jacobi directly on the columns of A or A^T, RSVD_ERR_UNSUPPORTED
 * above 4096); dtype F64 / F32.  Power (:183-219 with PM, src/PM.cpp): dtype F64, any n,
 * dim = r ? r : min(m, n) deflation steps, start vectors Philox(seed + i); stops at the first
 * sigma < 1e-12 (:198-208); *kept = triplets written (U, S, V columns 0..kept-1; V's columns are
 * the right singular vectors -- the reference's row layout is rebuilt by include/SVD_class.hpp).
 * Jacobi sets *kept = k without synchronising; Power synchronises the stream. */
int rsvd_svd(rsvd_handle_t h, int64_t m, int64_t n, const void *A, int64_t lda, int32_t dtype, int32_t method,
             int32_t r, uint64_t seed, void *U, int64_t ldu, void *S, void *V, int64_t ldv, int32_t *kept);
/* Device workspace bytes of rsvd_qr / rsvd_svd (for rsvd_set_workspace callers). */
int rsvd_qr_workspace_bytes(int64_t m, int64_t n, int32_t dtype, int32_t full, size_t *bytes);
int rsvd_svd_workspace_bytes(int64_t m, int64_t n, int32_t dtype, int32_t method, size_t *bytes);

/* ---- batched rSVD (ABI 7): many small matrices, or the tiles of one large matrix ----------- */

/* A batch of count0 * count1 matrices that share one rsvd_desc_t (m, n, lda, l, q, dtype, method,
 * seed, a_scale).  Matrix b = i0 + count0 * i1 starts at A + i0 * a_stride0 + i1 * a_stride1
 * (elements; the matrices may overlap) and writes U + b * u_stride, S + b * s_stride, V + b * v_stride.
 * A plain strided batch is count1 = 1.  The tm x tn tiles of a column-major m x n matrix (the block
 * decomposition of image_compression/src/image_com.cpp:350-371) are count0 = m / tm, a_stride0 = tm,
 * count1 = n / tn, a_stride1 = tn * lda with desc->m = tm, desc->n = tn. */
typedef struct {
    int64_t count0, count1;        /* batch = count0 * count1 matrices; matrix b = i0 + count0 * i1 */
    int64_t a_stride0, a_stride1;  /* elements: A_b = A + i0 * a_stride0 + i1 * a_stride1 (>= 0; may overlap) */
    int64_t omega_stride;          /* elements between Omega_b and Omega_b+1; 0 = one Omega shared by all */
    int64_t u_stride, s_stride, v_stride; /* elements between consecutive U_b / S_b / V_b (no overlap) */
} rsvd_batch_t;

/* Entry b is the rSVD rsvd_run computes on matrix b with seed desc->seed + b (omega == NULL: matrix b
 * draws Philox(desc->seed + b), the Omega of rsvd_generate_omega(n, l, seed + b, dtype)); U_b, S_b, V_b
 * are column-major with ldu / ldv as rsvd_run's.  Asynchronous on the handle's stream.
 * Fused path (rsvd_batched_is_fused == 1: dtype F64 / F32, l <= 64, l <= min(m, n), max(m, n) <= 256,
 * Jacobi / ParallelJacobi, qr_mode AUTO): ONE launch, one workgroup per matrix, A read in place (any
 * base and lda), panels orthonormalised by Householder reflectors, so rank-deficient matrices (zero
 * or constant tiles) come back with orthonormal U, V and zero trailing S like any other.  A matrix's
 * result depends only on its own inputs.  Everything else rsvd_run accepts (any dtype, l <= 4096,
 * larger matrices) loops rsvd_run over the sub-pointers on the same stream.
 * info (nullable, device, 2 words per matrix): info[2b] = Jacobi sweeps, info[2b + 1] bit 0 = a
 * rank-deficient sketch was met (looped path: the CGS2 repair ran), bit 1 = non-finite S.  On the
 * looped path a non-NULL info costs one synchronisation per matrix.  Non-finite S in any matrix
 * raises the handle's sticky word (rsvd_sync -> RSVD_ERR_NUMERICAL); the other matrices stay valid.
 * RSVD_ERR_INVALID_ARG: counts < 1, a negative stride, an output stride below its output (ldu * l,
 * l, ldv * l), ldu < m, ldv < n, flags != 0.  RSVD_ERR_UNSUPPORTED: a row-sharded handle (world > 1),
 * RSVD_SVD_POWER / RSVD_SVD_POWER_IC. */
int rsvd_run_batched(rsvd_handle_t h, const rsvd_desc_t *desc, const rsvd_batch_t *batch, const void *A,
                     const void *omega, int64_t ldo, void *U, int64_t ldu, void *S, void *V, int64_t ldv,
                     int32_t *info /* nullable, device, 2 per matrix */);
/* Device workspace bytes of rsvd_run_batched (leading dimensions unknown: ldu = m, ldv = n assumed
 * for the stride checks). */
int rsvd_batched_workspace_bytes(const rsvd_desc_t *desc, const rsvd_batch_t *batch, size_t *bytes);
/* Host-only: 1 when the description takes the fused kernel, 0 when it loops (or is invalid). */
int rsvd_batched_is_fused(const rsvd_desc_t *desc, const rsvd_batch_t *batch);

/* ---- rank-k compression (ABI 8): the rebuild and its error, fused into the batched rSVD ------ */

/* What every caller of the reference's rSVD does next: rebuild the low-rank matrix,
 * localMatrix = U * S.asDiagonal() * V.transpose() (image_compression/src/image_com.cpp:374,
 * Image::reconstruct :184-190), put each block back into the image (:381-394), and measure
 * ||A - U diag(S) V^T||_F (tests/rSVD_test.cpp:77-95).
 *   C_b   = U_b[:, :k] diag(S_b[:k]) V_b[:, :k]^T, 1 <= k <= min(l, n) (k = l is what the reference
 *           rebuilds), column-major with its own ldc, in the result dtype (fp64 for fp64 A, fp32 for
 *           every other A).  S carries |a_scale| and V its sign, so C approximates a_scale * A.
 *   err2  = two fp64 words per matrix, on the device: err2[2b] = ||a_scale A_b||_F^2 and
 *           err2[2b + 1] = ||a_scale A_b - C_b||_F^2 with C_b as stored (after rounding to its type).
 *           Both are fp64 sums in a fixed order (per thread, a 64-lane butterfly, waves and workgroups
 *           in index order; no atomics): bit-reproducible, independent of the grid, of the position
 *           in the batch and of the workspace's contents.
 * C_b = C + i0 * c_stride0 + i1 * c_stride1 (elements), as A_b in rsvd_batch_t.  The C blocks of a batch
 * must be pairwise disjoint; two layouts are accepted (a stride of a count of 1 is not looked at):
 *   tile grid      c_stride0 >= m, (count0 - 1) * c_stride0 + m <= ldc, c_stride1 >= n * ldc
 *   strided batch  c_stride0 >= (n - 1) * ldc + m and (count1 == 1 or c_stride1 >= count0 * c_stride0)
 * In place: C may be A itself -- same pointer, ldc == lda, the strides of A, A already of C's type (F64 /
 * F32); A's strides then fall under the same rule (overlapping tiles cannot be compressed in place).
 * Every element of A is read for the error and overwritten by the same thread, after the last
 * projection has finished with the tile.  Any other overlap of C with A is the caller's error. */
typedef struct {
    int32_t k, reserved;
    int64_t ldc, c_stride0, c_stride1;
} rsvd_compress_t;

/* rsvd_run_batched followed by the rebuild and the error of every matrix.  C nullable when err2 is set
 * (error only); U, S, V all NULL or all set; err2 nullable; info as rsvd_run_batched's.  The fused path is
 * taken exactly when rsvd_batched_is_fused(desc, batch) == 1 and is still ONE launch: the rebuild runs in
 * the workgroup that holds the matrix's factors in LDS, and with U = S = V = NULL the factors never reach
 * global memory.  U, S, V and info, where asked for, are bit-identical to rsvd_run_batched's.  Outside
 * the fused limits entry b is rsvd_run with seed + b followed by rsvd_lowrank, bit for bit, on the
 * handle's stream (factors the caller did not ask for live in the workspace).
 * RSVD_ERR_INVALID_ARG: what rsvd_run_batched refuses, k outside 1 .. min(l, n), ldc < m, a negative or
 * overlapping C stride, a partial set of U, S, V, C == A with another ldc / strides / a low-precision A.
 * RSVD_ERR_UNSUPPORTED: as rsvd_run_batched. */
int rsvd_compress_batched(rsvd_handle_t h, const rsvd_desc_t *desc, const rsvd_batch_t *batch,
                          const rsvd_compress_t *comp, const void *A, const void *omega, int64_t ldo,
                          void *C /* nullable if err2 */, void *U, int64_t ldu, void *S, void *V,
                          int64_t ldv /* U, S, V: all NULL or all set */,
                          double *err2 /* nullable, device, 2 per matrix */,
                          int32_t *info /* nullable, device, 2 per matrix */);
/* Host-only.  Device workspace bytes of rsvd_compress_batched (batch->u_stride / s_stride / v_stride are
 * not looked at).  Fused: exactly rsvd_batched_workspace_bytes (the tail needs no memory of its own);
 * looped: one rsvd_run, the error slots of rsvd_lowrank and one matrix's factors. */
int rsvd_compress_workspace_bytes(const rsvd_desc_t *desc, const rsvd_batch_t *batch, const rsvd_compress_t *comp,
                                  size_t *bytes);

/* C (m x n, ldc) = U[:, :k] diag(S[:k]) V[:, :k]^T for any m, n and k <= 4096 (MFMA, 64 x 64 tiles).
 * dtype F64 / F32 is the type of U (ldu >= m), S, V (ldv >= n) and C.  With A (m x n, lda, a_dtype F64 for
 * dtype F64, else F32 / BF16 / FP8_E4M3; the matrix is a_scale * A, a_scale 0 means 1) and err2 (device,
 * 2 fp64 words as above) the error is computed in the same pass.  C nullable when A and err2 are set
 * (error only, same words bit for bit); A nullable (no error; err2 must then be NULL).  C may be A
 * itself when A has C's type (each element is read and overwritten by one thread); U, S, V may not
 * overlap C.  Asynchronous on the handle's stream. */
int rsvd_lowrank(rsvd_handle_t h, int64_t m, int64_t n, int32_t k, int32_t dtype, const void *U, int64_t ldu,
                 const void *S, const void *V, int64_t ldv, void *C, int64_t ldc, const void *A, int64_t lda,
                 int32_t a_dtype, double a_scale, double *err2);
/* Host-only.  Device workspace bytes of rsvd_lowrank with an error (2 fp64 words per 64 x 64 tile of C). */
int rsvd_lowrank_workspace_bytes(int64_t m, int64_t n, size_t *bytes);

/* ---- POD (ABI 9): the snapshot method of the reference's class POD on the device --------------- */

/* POD modes of a tall snapshot matrix S (nh x ns, ns <= nh), POD.cpp:136-462 (standard_POD, energy_POD,
 * weight_POD; the ns > Nh branches are not covered).  Every step runs on the handle's stream:
 *   T = Xh S                    when Xh (symmetric, not checked; CSR) is given, else T = S
 *   C = D^1/2 S^T T D^1/2       ns x ns, ALWAYS fp64: fp32 S is widened on load (exact) and every product
 *                               and sum runs on the f64 MFMA, split over row chunks and summed in a fixed
 *                               order (no atomics), the lower triangle copied from the upper: C is
 *                               bitwise symmetric, bit-reproducible and independent of the workspace's
 *                               contents.  D = diag(d), d > 0 (NULL: ones); only diagonal D is supported
 *                               (the reference's only caller passes 0.1 I, Diff1D_openmp.cpp:229-231)
 *   small problem on C, fp64    svd_type (the reference's perform_SVD switch, POD.cpp:49-92):
 *                               1 / 2 = rsvd_svd(C, Jacobi) -- 2 too: rsvd_svd's ParallelJacobi follows the
 *                               reference's rotation path and its 1e-12 absolute stop, which leaves the
 *                               vectors ~1e-5 from the SVD's, and W divides them by sigma_i;
 *                               4 / 5 = rsvd_run(C, l = r, q, Jacobi / ParallelJacobi,
 *                               Omega = rsvd_generate_omega(ns, r, seed, F64));
 *                               0 / 3 (the power method) -> RSVD_ERR_UNSUPPORTED
 *   rank rule, POD.cpp:203-216  on the first r values: den = sum sigma_i^2,
 *                               while (I < 1 - tol^2 && N < r) { num += sigma_N^2; I = num / den; N++; }
 *                               den == 0 gives N = 0; tol = 1 gives N = 0
 *   W[:, i] = S D^1/2 V[:, i] / sigma_i, i < r (POD.cpp:172-174, :388-390); sigma_i == 0 -> a zero column
 * All r columns of W are written and N comes back as one device word: the host slices W[:, :N] (the
 * reference's conservativeResize).  Two quirks of the reference are the default: the modes are divided
 * by sigma_i(C) (so they have length 1 / sigma_i(S)) and the rule weighs by sigma_i(C)^2 = sigma_i(S)^4.
 * RSVD_POD_FLAG_TEXTBOOK divides by sqrt(sigma_i(C)) and weighs by sigma_i(C), as the book the reference
 * cites: W is then Xh-orthonormal and the rule is the usual sum of sigma_i(S)^2. */
#define RSVD_POD_FLAG_TEXTBOOK 1
typedef struct {
    int64_t nh, ns, lds;     /* S is nh x ns, column-major, lds >= nh; ns <= nh, ns <= 4096             */
    int32_t r;               /* modes computed, 1 .. ns (the reference's r)                               */
    int32_t dtype;           /* RSVD_F64 / RSVD_F32: type of S, Xh's values and W                         */
    int32_t svd_type;        /* the reference's 0..5 (POD.cpp:49-92); 1, 2, 4, 5 supported                */
    int32_t q;               /* power iterations of svd_type 4 / 5                                        */
    int32_t flags, reserved; /* RSVD_POD_FLAG_*                                                           */
    uint64_t seed;           /* Omega of svd_type 4 / 5 = rsvd_generate_omega(ns, r, seed, F64)           */
    double tol;              /* 0 <= tol <= 1                                                             */
} rsvd_pod_desc_t;
/* Xh in CSR, device pointers: rowptr nh + 1 entries, colind and val (S's type) nnz entries. */
typedef struct {
    const int32_t *rowptr, *colind;
    const void *val;
    int64_t nnz;
} rsvd_csr_t;

/* S is read in place: any lds >= nh, any element-aligned base.  W: nh x r, ldw >= nh, S's type; rows nh ..
 * ldw are not touched.  sigma: ns fp64 words on the device -- fp64 also for fp32 S, since they are the
 * singular values of the fp64 C: all ns (svd_type 1 / 2, the reference's sigma = getS()) or the first r
 * (4 / 5) are written, the rest zeroed.  N: one device int32.  C (nullable): ns x ns fp64, ld ns, the
 * weighted correlation matrix as the small solver saw it.  Asynchronous; nothing synchronises.
 * RSVD_ERR_INVALID_ARG: r outside 1 .. ns, lds < nh, ldw < nh, tol outside [0, 1] or NaN, svd_type outside
 * 0 .. 5, unknown flags, q < 0, NULL S / W / sigma / N, nnz < 0.  RSVD_ERR_UNSUPPORTED: ns > nh, ns > 4096,
 * svd_type 0 / 3, dtype BF16 / FP8_E4M3, a row-sharded handle. */
int rsvd_pod(rsvd_handle_t h, const rsvd_pod_desc_t *desc, const void *S, const rsvd_csr_t *Xh /* nullable */,
             const double *d /* nullable, device, ns */, void *W, int64_t ldw /* nh x r */,
             double *sigma /* device, ns words */, int32_t *N /* device, 1 word */,
             double *C /* nullable, device, ns x ns, ld ns */);
/* Host-only, with rsvd_pod's descriptor checks and codes.  Device workspace bytes of rsvd_pod: its own
 * region (T when has_xh, the chunk slabs, C, the small factors, Z) followed by the nested solver's. */
int rsvd_pod_workspace_bytes(const rsvd_pod_desc_t *desc, int has_xh, size_t *bytes);
/* Host-only.  The split of the correlation kernel: upper 32 x 32 block pairs of C and row chunks -- a
 * function of (nh, ns, dtype) alone. */
int rsvd_pod_plan(const rsvd_pod_desc_t *desc, int32_t *tiles, int32_t *chunks);

/* ---- host-pointer fp64 entry points used by the C++ drop-in headers (synchronous) --------- */
int rsvd_run_host_f64(rsvd_handle_t h, int64_t m, int64_t n, const double *A, int64_t lda, int32_t l,
                      int32_t q, int32_t method, const double *omega /* nullable, n x l, ld n */,
                      uint64_t seed, double *U /* m x d */, double *S /* d */, double *V /* n x d */);
int rsvd_range_finder_host_f64(rsvd_handle_t h, int64_t m, int64_t n, const double *A, int64_t lda,
                               const double *omega /* n x l, ld n */, int32_t l, int32_t q,
                               double *Q /* m x l */);
int rsvd_generate_omega_host_f64(rsvd_handle_t h, int64_t n, int32_t l, uint64_t seed, double *omega);
/* Q: m x (full ? m : n), ld m; R: (full ? m : n) x n, ld = its rows. */
int rsvd_qr_host_f64(rsvd_handle_t h, int64_t m, int64_t n, const double *A, int64_t lda, int32_t full, double *Q,
                     double *R);
/* U: m x min(m,n), S: min(m,n), V: n x min(m,n) buffers (ld m, n); *kept columns are written. */
int rsvd_svd_host_f64(rsvd_handle_t h, int64_t m, int64_t n, const double *A, int64_t lda, int32_t method, int32_t r,
                      uint64_t seed, double *U, double *S, double *V, int32_t *kept);
/* Image::compress_parallel's numeric core on host buffers: every tile_m x tile_n tile of A (tile_m =
 * tile_n = 0: the whole matrix as one tile; the tiles must divide it) is replaced by its rank-k rebuild
 * from an rSVD of width l with q power iterations, Omega = Philox(seed + i + (m / tile_m) * j) for tile
 * (i, j).  C: m x n, ldc (may be A).  err2 (host, nullable): the two words of rsvd_compress_batched per
 * tile, tile (i, j) at 2 * (i + (m / tile_m) * j). */
int rsvd_compress_host_f64(rsvd_handle_t h, int64_t m, int64_t n, const double *A, int64_t lda, int32_t tile_m,
                           int32_t tile_n, int32_t l, int32_t k, int32_t q, uint64_t seed, double *C, int64_t ldc,
                           double *err2 /* host, 2 per tile, nullable */);

/* class POD's numeric core on host buffers (include/POD.hpp): S nh x ns (ld desc->lds), Xh as host CSR
 * (rowptr NULL: none), d host (nullable); desc->dtype is taken as RSVD_F64.  W: nh x r, ld nh (all r
 * columns), sigma: ns, *N: the rank rule's N. */
int rsvd_pod_host_f64(rsvd_handle_t h, const rsvd_pod_desc_t *desc, const double *S, const int32_t *rowptr,
                      const int32_t *colind, const double *val, int64_t nnz, const double *d /* nullable, ns */,
                      double *W, double *sigma, int32_t *N);

#ifdef __cplusplus
}
#endif
#endif /* RSVD_C_H */
