// lowrank.hip -- the rank-k rebuild C = U_k diag(S_k) V_k^T of Image::reconstruct
// (image_compression/src/image_com.cpp:184-190, :374) for any m, n and k, with the error of
// tests/rSVD_test.cpp:77-95 fused into its epilogue.
//
// 64 x 64 output tile per 256-thread workgroup (4 waves, 32 x 32 each = 2 x 2 MFMA tiles) on
// v_mfma_f64_16x16x4f64 / v_mfma_f32_16x16x4f32, as gemm.hip.  The 64 x 16 slices of U diag(S) and of V
// go through LDS k-major (Us[k][i], Vs[k][j], pitch 68: the operand of lane (r, h) at k-step kk is
// Xs[4 kk + h][.. + r], one bank-conflict-free read); both are read from global memory along their
// contiguous dimension and U is scaled by S on the way in.  The MFMA gets V as its row operand and
// U diag(S) as its column operand, so a lane's accumulator register holds C[i = .. + r, j = .. + row(h, q)]:
// the 16 lanes of a row group store, and read A at, 16 consecutive elements of one column.
//
// Small k makes this a stream over C and A, so each is touched once: the thread that owns C[i, j]
// reads A[i, j] (fp64, fp32, bf16 or e4m3, times a_scale) before it stores -- C may be A itself -- and
// adds a^2 and (a - c)^2, c as rounded to its type, to two fp64 sums.  Those are joined in a fixed
// order (per thread, the 64-lane butterfly, the four waves in index order) into the workgroup's slot of
// the workspace, and a second one-workgroup kernel sums the slots: thread t takes slots t, t + 256, ..
// in index order, then the same join.  No atomics; the words depend on m, n, k and the data alone.
#include "common.hpp"
#include "lowrank.hpp"

namespace rsvd {

namespace {

constexpr int LT = 64, LK = 16, LPI = LT + 4;  // tile, k slice, LDS pitch

// OCP e4m3fn -> fp32 (exact): 1 sign, 4 exponent (bias 7), 3 mantissa bits; S.1111.111 is NaN
__device__ __forceinline__ float lr_e4m3_to_f32(uint32_t b) {
    const uint32_t e = (b >> 3) & 15u, mt = b & 7u;
    float v;
    if (e == 15u && mt == 7u) v = __builtin_nanf("");
    else if (e == 0u) v = (float)mt * 0x1p-9f;
    else v = __uint_as_float(((e + 120u) << 23) | (mt << 20));
    return (b & 0x80u) ? -v : v;
}

// element o of A as stored (adt: 0 f64, 1 f32, 2 bf16, 3 e4m3), widened exactly to fp64
__device__ __forceinline__ double load_a(const void* A, int adt, int64_t o) {
    switch (adt) {
        case 0: return reinterpret_cast<const double*>(A)[o];
        case 1: return (double)reinterpret_cast<const float*>(A)[o];
        case 2: return (double)__uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(A)[o] << 16);
        default: return (double)lr_e4m3_to_f32(reinterpret_cast<const uint8_t*>(A)[o]);
    }
}

// the workgroup's two fp64 sums, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ void block_join(double& sa, double& se, double* part) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    sa = warp_sum(sa);
    se = warp_sum(se);
    if (lane == 0) {
        part[2 * w] = sa;
        part[2 * w + 1] = se;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sa = part[0];
        se = part[1];
        for (int t = 1; t < 4; ++t) {
            sa += part[2 * t];
            se += part[2 * t + 1];
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void lowrank_kernel(int64_t M, int64_t N, int K, const T* U, int64_t ldu, const T* S,
                                                      const T* V, int64_t ldv, T* C, int64_t ldc, const void* A,
                                                      int64_t lda, int adt, double a_scale, double* slots) {
#pragma clang fp contract(off)  // a_scale a is rounded to fp64 before c, as stored, is taken from it
    typedef Mfma<T> MM;
    __shared__ T Us[LK][LPI];
    __shared__ T Vs[LK][LPI];
    __shared__ double part[8];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 15, h = lane >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * LT, j0 = (int64_t)blockIdx.y * LT;
    const int wi = (w >> 1) * 32, wj = (w & 1) * 32;
    typename MM::acc_t acc[2][2];  // [j block][i block]
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = MM::zero();
    for (int k0 = 0; k0 < K; k0 += LK) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // threads along i (U) and along j (V): both contiguous in memory
            const int e = tid + 256 * u;
            const int x = e & 63, kk = e >> 6;
            const int gk = k0 + kk;
            T uv = T(0), vv = T(0);
            if (gk < K) {
                if (i0 + x < M) uv = U[i0 + x + (int64_t)gk * ldu] * S[gk];
                if (j0 + x < N) vv = V[j0 + x + (int64_t)gk * ldv];
            }
            Us[kk][x] = uv;
            Vs[kk][x] = vv;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < LK / 4; ++kk) {
            const T u0 = Us[4 * kk + h][wi + r], u1 = Us[4 * kk + h][wi + 16 + r];
            const T v0 = Vs[4 * kk + h][wj + r], v1 = Vs[4 * kk + h][wj + 16 + r];
            acc[0][0] = MM::mma(v0, u0, acc[0][0]);
            acc[0][1] = MM::mma(v0, u1, acc[0][1]);
            acc[1][0] = MM::mma(v1, u0, acc[1][0]);
            acc[1][1] = MM::mma(v1, u1, acc[1][1]);
        }
        __syncthreads();
    }
    double sa = 0.0, se = 0.0;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t gj = j0 + wj + 16 * a + MM::row(h, q), gi = i0 + wi + 16 * b + r;
                if (gi < M && gj < N) {
                    const T cv = acc[a][b][q];
                    if (A) {
                        const double av = load_a(A, adt, gi + gj * lda) * a_scale;
                        const double d = av - (double)cv;
                        sa = fma(av, av, sa);
                        se = fma(d, d, se);
                    }
                    if (C) C[gi + gj * ldc] = cv;
                }
            }
    if (!slots) return;
    block_join(sa, se, part);
    if (tid == 0) {
        const int64_t tile = blockIdx.x + (int64_t)gridDim.x * blockIdx.y;
        slots[2 * tile] = sa;
        slots[2 * tile + 1] = se;
    }
}

__global__ __launch_bounds__(256) void lowrank_err_kernel(const double* slots, int64_t tiles, double* err2) {
    __shared__ double part[8];
    double sa = 0.0, se = 0.0;
    for (int64_t t = threadIdx.x; t < tiles; t += 256) {
        sa += slots[2 * t];
        se += slots[2 * t + 1];
    }
    block_join(sa, se, part);
    if (threadIdx.x == 0) {
        err2[0] = sa;
        err2[1] = se;
    }
}

}  // namespace

int64_t lowrank_tiles(int64_t m, int64_t n) { return ((m + LT - 1) / LT) * ((n + LT - 1) / LT); }

hipError_t launch_lowrank(int dtype, int64_t m, int64_t n, int k, const void* U, int64_t ldu, const void* S,
                          const void* V, int64_t ldv, void* C, int64_t ldc, const void* A, int64_t lda, int a_dtype,
                          double a_scale, double* slots, double* err2, hipStream_t s) {
    const dim3 grid((unsigned)((m + LT - 1) / LT), (unsigned)((n + LT - 1) / LT));
    const bool err = A && err2;
    if (dtype == 0)
        hipLaunchKernelGGL((lowrank_kernel<double>), grid, dim3(256), 0, s, m, n, k, static_cast<const double*>(U), ldu,
                           static_cast<const double*>(S), static_cast<const double*>(V), ldv, static_cast<double*>(C),
                           ldc, err ? A : nullptr, lda, a_dtype, a_scale, err ? slots : nullptr);
    else
        hipLaunchKernelGGL((lowrank_kernel<float>), grid, dim3(256), 0, s, m, n, k, static_cast<const float*>(U), ldu,
                           static_cast<const float*>(S), static_cast<const float*>(V), ldv, static_cast<float*>(C), ldc,
                           err ? A : nullptr, lda, a_dtype, a_scale, err ? slots : nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !err) return e;
    hipLaunchKernelGGL(lowrank_err_kernel, dim3(1), dim3(256), 0, s, slots, lowrank_tiles(m, n), err2);
    return hipGetLastError();
}

}  // namespace rsvd
