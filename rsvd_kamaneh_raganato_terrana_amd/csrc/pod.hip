// pod.hip -- device side of the snapshot-method POD (include/rsvd_c.h rsvd_pod; POD.cpp:136-462 of the
// reference): the split-K fp64 correlation C = D^1/2 S^T T D^1/2 of a tall column-major snapshot matrix,
// the CSR product T = Xh S in front of it, and the one-workgroup tail (rank rule, Z = D^1/2 V diag(1 / sigma)).
#include "common.hpp"
#include "pod.hpp"

namespace rsvd {

namespace {

typedef Mfma<double> MD;

// A lane's share of one k-step: 32 contiguous bytes of one column (8 floats / 4 doubles), so the four
// lane groups h = 0 .. 3 of a column read one 128-B line and a step covers RS = 4 SEG rows.
template <typename T> struct PodSeg {
    static constexpr int SEG = 32 / (int)sizeof(T), RS = 4 * SEG;
};

// rows [row, row + SEG) of the column at `col`, zero past `end`.  16-B loads when the column is 16-B
// aligned (vec) and the segment lies inside the chunk, element loads otherwise: the values and their k
// slots are the same either way, so the sums do not depend on the alignment of the caller's S.
template <typename T, int SEG>
__device__ __forceinline__ void pod_load_seg(const T* __restrict__ col, int64_t row, int64_t end, bool vec,
                                             T (&out)[SEG]) {
    constexpr int VE = Vec16<T>::N;
    typedef typename Vec16<T>::type V;
    if (vec && row + SEG <= end) {
#pragma unroll
        for (int v = 0; v < SEG / VE; ++v) {
            const V x = *reinterpret_cast<const V*>(col + row + VE * v);
#pragma unroll
            for (int e = 0; e < VE; ++e) out[VE * v + e] = Vec16<T>::get(x, e);
        }
    } else {
#pragma unroll
        for (int e = 0; e < SEG; ++e) out[e] = row + e < end ? col[row + e] : T(0);
    }
}

// (a, b), a <= b, of upper block pair blk (row-major over the upper triangle of nb x nb blocks)
__device__ __forceinline__ void pod_block_of(int blk, int nb, int& a, int& b) {
    int rem = blk;
    a = 0;
    while (rem >= nb - a) {
        rem -= nb - a;
        ++a;
    }
    b = a + rem;
}

// One wave per (32 x 32 block pair of C, row chunk), as gram_wide_kernel -- but on the caller's
// column-major S: lane (r, h) of an MFMA holds the element of column c0 + r for k slot h, and which
// row a k slot stands for is free as long as both operands agree, so the lane takes rows
// i0 + SEG h .. + SEG - 1 of its column in one contiguous read and feeds them to SEG MFMAs.  fp32 is
// widened on load (exact); every product and sum runs on v_mfma_f64_16x16x4_f64.  Consecutive waves
// take the block pairs of ONE chunk, so the nb + 1 reads of a chunk's rows meet in L2.
// TT is the type of T: S's when T is S itself, fp64 for T = Xh S (pod_spmm_kernel).
template <typename T, typename TT>
__global__ __launch_bounds__(256) void pod_corr_kernel(const T* __restrict__ S, int64_t lds, const TT* __restrict__ Tm,
                                                       int64_t ldt, int64_t nh, int ns, int nblk, int nchunk,
                                                       int64_t rpc, int vec_s, int vec_t,
                                                       double* __restrict__ slabs) {
    constexpr int SEG = PodSeg<T>::SEG, RS = PodSeg<T>::RS;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int blk = gw % nblk, chunk = gw / nblk;
    if (chunk >= nchunk) return;
    int a, b;
    pod_block_of(blk, (ns + 31) / 32, a, b);
    const int r = lane & 15, h = lane >> 4;
    const int ca = 32 * a + r, cb = 32 * b + r;
    const bool oka0 = ca < ns, oka1 = ca + 16 < ns, okb0 = cb < ns, okb1 = cb + 16 < ns;
    // (columns past ns are never addressed: their pointers stay on column 0)
    const T* pa0 = S + (oka0 ? (int64_t)ca * lds : 0);
    const T* pa1 = S + (oka1 ? (int64_t)(ca + 16) * lds : 0);
    const TT* pb0 = Tm + (okb0 ? (int64_t)cb * ldt : 0);
    const TT* pb1 = Tm + (okb1 ? (int64_t)(cb + 16) * ldt : 0);
    const int64_t beg = (int64_t)chunk * rpc;
    const int64_t end = (beg + rpc < nh) ? beg + rpc : nh;
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = MD::zero();
    for (int64_t i0 = beg; i0 < end; i0 += RS) {
        const int64_t row = i0 + SEG * h;
        T va0[SEG], va1[SEG];
        TT vb0[SEG], vb1[SEG];
#pragma unroll
        for (int e = 0; e < SEG; ++e) {
            va0[e] = va1[e] = T(0);
            vb0[e] = vb1[e] = TT(0);
        }
        if (row < end) {
            if (oka0) pod_load_seg<T, SEG>(pa0, row, end, vec_s != 0, va0);
            if (oka1) pod_load_seg<T, SEG>(pa1, row, end, vec_s != 0, va1);
            if (okb0) pod_load_seg<TT, SEG>(pb0, row, end, vec_t != 0, vb0);
            if (okb1) pod_load_seg<TT, SEG>(pb1, row, end, vec_t != 0, vb1);
        }
#pragma unroll
        for (int e = 0; e < SEG; ++e) {
            const double a0 = (double)va0[e], a1 = (double)va1[e];
            const double b0 = (double)vb0[e], b1 = (double)vb1[e];
            acc[0][0] = MD::mma(a0, b0, acc[0][0]);
            acc[0][1] = MD::mma(a0, b1, acc[0][1]);
            acc[1][0] = MD::mma(a1, b0, acc[1][0]);
            acc[1][1] = MD::mma(a1, b1, acc[1][1]);
        }
    }
    // every (chunk, block) slab is written in full: nothing of the workspace's old contents survives
    double* dst = slabs + ((int64_t)chunk * nblk + blk) * 1024;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[(16 * x + MD::row(h, j)) * 32 + 16 * y + r] = acc[x][y][j];
}

// The chunk partials of every entry summed in a fixed order (the scheme of gram_reduce4_kernel: 64
// entries x 4 chunk ranges per workgroup, the ranges combined in wave order), scaled by sqrt(d_i d_j)
// and written to both triangles from the upper one -- also inside a diagonal block, whose lower half
// is not read: with T = Xh S the two halves differ in the last bits, and C has to be symmetric.
__global__ __launch_bounds__(256) void pod_reduce_kernel(const double* __restrict__ slabs, int nblk, int nchunk, int ns,
                                                         const double* __restrict__ d, double* __restrict__ C,
                                                         double* __restrict__ C2) {
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int64_t e = blockIdx.x * (int64_t)64 + lane;
    bool ok = e < (int64_t)nblk * 1024;
    const int blk = ok ? (int)(e / 1024) : 0, loc = (int)(e % 1024);
    int a, b;
    pod_block_of(blk, (ns + 31) / 32, a, b);
    const int li = loc / 32, lj = loc % 32;
    const int ra = 32 * a + li, cb = 32 * b + lj;
    ok = ok && ra < ns && cb < ns && !(a == b && li > lj);
    double sum = 0.0;
    if (ok) {
        const int64_t cs = (int64_t)nblk * 1024;
        const double* src = slabs + (int64_t)blk * 1024 + loc;
        const int c0 = (int)((int64_t)nchunk * k / 4), c1 = (int)((int64_t)nchunk * (k + 1) / 4);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        int c = c0;
        for (; c + 4 <= c1; c += 4) {
            s0 += src[(c + 0) * cs];
            s1 += src[(c + 1) * cs];
            s2 += src[(c + 2) * cs];
            s3 += src[(c + 3) * cs];
        }
        for (; c < c1; ++c) s0 += src[c * cs];
        sum = (s0 + s1) + (s2 + s3);
    }
    part[k][lane] = sum;
    __syncthreads();
    if (k == 0 && ok) {
        double t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        if (d) t *= sqrt(d[ra] * d[cb]);
        C[(int64_t)cb * ns + ra] = t;
        if (ra != cb) C[(int64_t)ra * ns + cb] = t;
        if (C2) {
            C2[(int64_t)cb * ns + ra] = t;
            if (ra != cb) C2[(int64_t)ra * ns + cb] = t;
        }
    }
}

// T = Xh S: lanes on consecutive rows (a banded Xh reads a column of S coalesced), blockIdx.y on groups
// of 8 columns.  A row's sum runs in storage order in fp64 and is stored in fp64 whatever S's type:
// rounded to fp32, T would carry 2^-24 relative errors straight into C, which is kept to fp64 accuracy.
// Entries outside the matrix are skipped.
template <typename T>
__global__ __launch_bounds__(256) void pod_spmm_kernel(const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ colind, const T* __restrict__ val,
                                                       int64_t nnz, int64_t nh, int ns, const T* __restrict__ S,
                                                       int64_t lds, double* __restrict__ Tm) {
    const int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x;
    if (i >= nh) return;
    int64_t k0 = rowptr[i], k1 = rowptr[i + 1];
    if (k0 < 0) k0 = 0;
    if (k1 > nnz) k1 = nnz;
    const int j0 = blockIdx.y * 8, j1 = j0 + 8 < ns ? j0 + 8 : ns;
    for (int j = j0; j < j1; ++j) {
        const T* col = S + (int64_t)j * lds;
        double sum = 0.0;
        for (int64_t k = k0; k < k1; ++k) {
            const int64_t c = colind[k];
            if (c >= 0 && c < nh) sum += (double)val[k] * (double)col[c];
        }
        Tm[(int64_t)j * nh + i] = sum;
    }
}

// The reference's rank rule (POD.cpp:203-216) on sigma[0 .. r) by one thread, Z by all.
template <typename T>
__global__ __launch_bounds__(256) void pod_finish_kernel(const double* __restrict__ V, int64_t ldv, int ns, int r,
                                                         int nsig, const double* __restrict__ d, double tol,
                                                         int textbook, double* __restrict__ sigma,
                                                         int32_t* __restrict__ N, T* __restrict__ Z) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        double den = 0.0;
        for (int i = 0; i < r; ++i) den += textbook ? sigma[i] : sigma[i] * sigma[i];
        int n = 0;
        if (den != 0.0) {  // a zero spectrum keeps no mode
            const double thr = 1.0 - tol * tol;
            double I = 0.0, num = 0.0;
            while (I < thr && n < r) {
                num += textbook ? sigma[n] : sigma[n] * sigma[n];
                I = num / den;
                ++n;
            }
        }
        *N = n;
    }
    for (int64_t idx = tid; idx < (int64_t)ns * r; idx += 256) {
        const int j = (int)(idx % ns), i = (int)(idx / ns);
        const double sg = sigma[i];
        double z = 0.0;
        if (sg > 0.0) z = (d ? sqrt(d[j]) : 1.0) * V[(int64_t)i * ldv + j] / (textbook ? sqrt(sg) : sg);
        Z[idx] = (T)z;
    }
    __syncthreads();
    for (int i = nsig + tid; i < ns; i += 256) sigma[i] = 0.0;
}

template <typename T> bool pod_vec_ok(const void* p, int64_t ld) {
    return reinterpret_cast<uintptr_t>(p) % 16 == 0 && (ld * (int64_t)sizeof(T)) % 16 == 0;
}

}  // namespace

PodPlan plan_pod_corr(int64_t nh, int64_t ns, int dtype) {
    (void)dtype;  // both types split alike (the chunk edges are multiples of either step)
    PodPlan p;
    const int64_t nb = (ns + 31) / 32;
    p.blocks = (int)(nb * (nb + 1) / 2);
    // ~4096 waves (16 per CU) where the rows allow it, >= 256 rows per chunk, <= 512 chunks
    int64_t chunks = (4096 + p.blocks - 1) / p.blocks;
    const int64_t max_by_rows = (nh + 255) / 256;
    if (chunks > max_by_rows) chunks = max_by_rows;
    if (chunks > 512) chunks = 512;
    if (chunks < 1) chunks = 1;
    int64_t rpc = (nh + chunks - 1) / chunks;
    rpc = (rpc + 31) / 32 * 32;
    p.rows_per_chunk = rpc;
    p.chunks = (int)((nh + rpc - 1) / rpc);
    if (p.chunks < 1) p.chunks = 1;
    return p;
}

hipError_t launch_pod_corr(int dtype, const void* S, int64_t lds, const void* T, int t_f64, int64_t ldt, int64_t nh,
                           int64_t ns, const PodPlan& p, const double* d, double* slabs, double* C, double* C2,
                           hipStream_t s) {
    const int waves = p.blocks * p.chunks;
    const dim3 grid((unsigned)((waves + 3) / 4));
    auto go = [&](auto ts, auto tt) {
        typedef decltype(ts) TS;
        typedef decltype(tt) TT;
        hipLaunchKernelGGL((pod_corr_kernel<TS, TT>), grid, dim3(256), 0, s, static_cast<const TS*>(S), lds,
                           static_cast<const TT*>(T), ldt, nh, (int)ns, p.blocks, p.chunks, p.rows_per_chunk,
                           (int)pod_vec_ok<TS>(S, lds), (int)pod_vec_ok<TT>(T, ldt), slabs);
    };
    if (dtype == 0) go(double(0), double(0));
    else if (t_f64) go(float(0), double(0));
    else go(float(0), float(0));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t tot = (int64_t)p.blocks * 1024;
    hipLaunchKernelGGL(pod_reduce_kernel, dim3((unsigned)((tot + 63) / 64)), dim3(256), 0, s, slabs, p.blocks, p.chunks,
                       (int)ns, d, C, C2);
    return hipGetLastError();
}

hipError_t launch_pod_spmm(int dtype, const int32_t* rowptr, const int32_t* colind, const void* val, int64_t nnz,
                           int64_t nh, int64_t ns, const void* S, int64_t lds, double* T, hipStream_t s) {
    const dim3 grid((unsigned)((nh + 255) / 256), (unsigned)((ns + 7) / 8));
    if (dtype == 0)
        hipLaunchKernelGGL((pod_spmm_kernel<double>), grid, dim3(256), 0, s, rowptr, colind,
                           static_cast<const double*>(val), nnz, nh, (int)ns, static_cast<const double*>(S), lds,
                           T);
    else
        hipLaunchKernelGGL((pod_spmm_kernel<float>), grid, dim3(256), 0, s, rowptr, colind,
                           static_cast<const float*>(val), nnz, nh, (int)ns, static_cast<const float*>(S), lds, T);
    return hipGetLastError();
}

hipError_t launch_pod_finish(int dtype, const double* V, int64_t ldv, int ns, int r, int nsig, const double* d,
                             double tol, int textbook, double* sigma, int32_t* N, void* Z, hipStream_t s) {
    if (dtype == 0)
        hipLaunchKernelGGL((pod_finish_kernel<double>), dim3(1), dim3(256), 0, s, V, ldv, ns, r, nsig, d, tol, textbook,
                           sigma, N, static_cast<double*>(Z));
    else
        hipLaunchKernelGGL((pod_finish_kernel<float>), dim3(1), dim3(256), 0, s, V, ldv, ns, r, nsig, d, tol, textbook,
                           sigma, N, static_cast<float*>(Z));
    return hipGetLastError();
}

}  // namespace rsvd
