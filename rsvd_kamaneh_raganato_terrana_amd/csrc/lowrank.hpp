// lowrank.hpp -- the rank-k rebuild C = U_k diag(S_k) V_k^T with its fused error (lowrank.hip), behind
// rsvd_lowrank and the looped path of rsvd_compress_batched.  Private to librsvd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsvd {

// 64 x 64 output tiles of an m x n C: the error kernel's workspace is 2 fp64 words per tile.
int64_t lowrank_tiles(int64_t m, int64_t n);
// dtype (0 = f64, 1 = f32) is the type of U, S, V and C; a_dtype (rsvd_dtype_t) that of A.  C nullable
// (error only); A, slots and err2 nullable together (no error).  C may be A itself.
hipError_t launch_lowrank(int dtype, int64_t m, int64_t n, int k, const void* U, int64_t ldu, const void* S,
                          const void* V, int64_t ldv, void* C, int64_t ldc, const void* A, int64_t lda, int a_dtype,
                          double a_scale, double* slots, double* err2, hipStream_t s);

}  // namespace rsvd
