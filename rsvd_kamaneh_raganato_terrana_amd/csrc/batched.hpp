// batched.hpp -- the fused batched rSVD (batched.hip: one workgroup per matrix, one launch per batch)
// and the limits its host side (batched_run.cpp) plans with.  Private to librsvd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rsvd {

constexpr int kBatchedMaxDim = 256;            // max(m, n) of a fused matrix
constexpr int kBatchedMaxL = 64;               // sketch width of a fused matrix
constexpr size_t kBatchedLdsBudget = 163840;   // 160 KiB of LDS per workgroup (gfx950)
constexpr int kBatchedMaxGrid = 1024;          // workgroups of one launch; each walks b, b + grid, ...

// One launch's arguments.  Every matrix has the sizes m, n, l, q; matrix b = i0 + count0 * i1 reads
// A + i0 * a_stride0 + i1 * a_stride1 (elements) and writes U + b * u_stride, S + b * s_stride,
// V + b * v_stride.  omega == nullptr: Philox(seed + b).
// Compression (launch_batched_compress): the rank-k rebuild C_b = C + i0 * c_stride0 + i1 * c_stride1
// (nullable) and the two fp64 error words err2 + 2 b (nullable); U, S, V may then all be nullptr.
struct BatchedArgs {
    const void* A;
    const void* omega;
    void* U;
    void* S;
    void* V;
    int32_t* info;     // nullable: 2 words per matrix (sweeps; bit 0 rank deficiency met, bit 1 non-finite)
    int* nonfinite;    // the handle's sticky non-finite word
    char* ws;          // panel slices (ws_slice bytes per workgroup) when the panels do not fit in LDS
    size_t ws_slice;
    int64_t batch, count0, a_stride0, a_stride1, omega_stride, u_stride, s_stride, v_stride;
    int64_t lda, ldo, ldu, ldv;
    int m, n, l, q;
    uint64_t seed;
    double s_scale;    // |a_scale|
    int v_neg;         // a_scale < 0: V changes sign
    // the compress tail (batched_rsvd_kernel<.., COMP = true> only)
    void* C;           // nullable: C_b in T, column-major ldc; may be A itself (in place)
    double* err2;      // nullable: err2[2b] = ||a_scale A_b||_F^2, err2[2b + 1] = ||a_scale A_b - C_b||_F^2
    int64_t ldc, c_stride0, c_stride1;
    int k;             // 1 <= k <= l
};

// LDS bytes of the l x l area (Jacobi columns, U_w, the reflector scalars) for dtype (0 = f64, 1 = f32).
size_t batched_small_bytes(int dtype, int LP);
// Bytes of the two l-wide panels (m x l and n x l, column-major) of one matrix.
size_t batched_panel_bytes(int dtype, int m, int n, int l);
// panels_in_lds: the panels sit behind the l x l area in LDS (lds_bytes covers both); otherwise in
// workgroup blockIdx.x's slice of a.ws.
hipError_t launch_batched_rsvd(const BatchedArgs& a, int dtype, int LP, bool panels_in_lds, size_t lds_bytes, int grid,
                               hipStream_t s);
// The same launch with the compress tail: the factors are written only when a.U is set, then the
// rank-a.k rebuild and its error words (same LDS and workspace as launch_batched_rsvd).
hipError_t launch_batched_compress(const BatchedArgs& a, int dtype, int LP, bool panels_in_lds, size_t lds_bytes,
                                   int grid, hipStream_t s);

}  // namespace rsvd
