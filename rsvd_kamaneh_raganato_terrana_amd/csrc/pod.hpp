// pod.hpp -- launch wrappers of pod.hip (the snapshot-method POD behind rsvd_pod, pod.cpp).
// Private to librsvd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rsvd {

// The split of the correlation C = S^T T (ns x ns) over (upper 32 x 32 block pairs) x (row chunks):
// a pure function of (nh, ns, dtype), so the summation order -- and with it every bit of C -- is too.
struct PodPlan {
    int blocks;              // upper-triangle 32 x 32 block pairs of C
    int chunks;              // row chunks (K splits)
    int64_t rows_per_chunk;  // a multiple of 32
};
PodPlan plan_pod_corr(int64_t nh, int64_t ns, int dtype);
inline size_t pod_slab_bytes(const PodPlan& p) { return sizeof(double) * 1024 * (size_t)p.blocks * p.chunks; }

// C (ns x ns fp64, ld ns; C2 nullable: a second copy) = sqrt(d_i d_j) (S^T T)_ij, both triangles from the
// upper one.  S, T: nh x ns column-major (lds, ldt >= nh), read in place from any element-aligned base;
// dtype 0 = f64, 1 = f32 is S's type, T is S itself (t_f64 = 0) or fp64 (t_f64 = 1, launch_pod_spmm's).
// d nullable (ones).  slabs: pod_slab_bytes(p).
hipError_t launch_pod_corr(int dtype, const void* S, int64_t lds, const void* T, int t_f64, int64_t ldt, int64_t nh,
                           int64_t ns, const PodPlan& p, const double* d, double* slabs, double* C, double* C2,
                           hipStream_t s);

// T (nh x ns fp64, ld nh) = Xh S for a CSR Xh (nh rows, nnz entries; values in S's type), fp64 row sums in
// storage order, kept in fp64.  Row ranges are clipped to [0, nnz) and column indices outside [0, nh) skipped.
hipError_t launch_pod_spmm(int dtype, const int32_t* rowptr, const int32_t* colind, const void* val, int64_t nnz,
                           int64_t nh, int64_t ns, const void* S, int64_t lds, double* T, hipStream_t s);

// One workgroup: the rank rule on sigma[0 .. r) -> *N, Z (ns x r, ld ns, S's type) = D^1/2 V[:, :r] diag(1 / sigma)
// (1 / sqrt(sigma) and the sigma-weighted rule when textbook), sigma[nsig .. ns) = 0.
hipError_t launch_pod_finish(int dtype, const double* V, int64_t ldv, int ns, int r, int nsig, const double* d,
                             double tol, int textbook, double* sigma, int32_t* N, void* Z, hipStream_t s);

}  // namespace rsvd
