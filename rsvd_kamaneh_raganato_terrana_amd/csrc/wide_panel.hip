// wide_panel.hip -- Q = P R^-1 and the other panel products of the wide engine's CholeskyQR (wide.hpp), and
// its elementwise kernels: repair, bf16 split, the low-precision Omega, bf16 -> e4m3, convert / scale.
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "wide_dev.hpp"

namespace rsvd {

namespace {

// ------------------------------------------------------------------------------------------------
// Out = In * M.  Workgroup = 64 rows x CT columns (4 waves x 16 rows; LP > CT -> column blocks,
// adjacent on one XCD so In rows are re-read from L2).  K runs in chunks staged through LDS with
// 16-B loads of M (given in T precision); a lane's In vector (float4 / double2) feeds VW MFMAs
// (k-slot h of MFMA t <-> k = k0 + VW h + t), the chunk's In vectors are loaded before the M
// staging so their latency overlaps it.  fp32: v_mfma_f32_16x16x4_f32; fp64: the f64 form.
// Upper-triangular M (R^-1): K stops at the block's last column (no per-tile skipping inside the
// unrolled MFMA loop: a data-dependent skip there makes hipcc shuffle the accumulators).
template <typename T> struct PG;
template <> struct PG<float> {
    typedef float4 V;
    static constexpr int VW = 4, PAD = 4;  // pitch CT+4: the two k-rows of a half-wave hit disjoint banks
    typedef Mfma<float> M;
};
template <> struct PG<double> {
    typedef double2 V;
    static constexpr int VW = 2, PAD = 8;
    typedef Mfma<double> M;
};


template <typename T, int CT>
__global__ __launch_bounds__(256) void panel_gemm_kernel(const T* __restrict__ In, int64_t rows, int LP,
                                                         const T* __restrict__ Mm, int upper, T* __restrict__ Out,
                                                         int64_t ldo, int cols, bf16_t* __restrict__ hi,
                                                         bf16_t* __restrict__ lo, int ncb,
                                                         const int* __restrict__ pred) {
    if (pred && *pred == 0) return;
    typedef PG<T> C;
    typedef typename C::M M;
    typedef typename C::V V;
    constexpr int VW = C::VW;
    constexpr int G = CT / 16;
    constexpr int NJ = 4;             // k-steps of 4 VW per chunk
    constexpr int KC = NJ * 4 * VW;   // 64 (fp32) / 32 (fp64)
    constexpr int MP = CT + C::PAD;   // LDS pitch of the M chunk
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* Ms = reinterpret_cast<T*>(smem_raw);  // [KC][MP]
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, h = lane >> 4;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int cb = bid % ncb;
    const int64_t row0 = (int64_t)(bid / ncb) * 64;
    const int c0 = cb * CT;
    const int64_t row = row0 + 16 * w + r;
    const bool rok = row < rows;
    const int kmax = upper ? ((c0 + CT < LP) ? c0 + CT : LP) : LP;
    typename M::acc_t acc[G];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g] = M::zero();
    for (int kc = 0; kc < kmax; kc += KC) {
        V a[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k = kc + 4 * VW * j + VW * h;
            if (rok && k < LP) {
                a[j] = *reinterpret_cast<const V*>(In + row * LP + k);
            } else {
                T* e = reinterpret_cast<T*>(&a[j]);
#pragma unroll
                for (int t = 0; t < VW; ++t) e[t] = T(0);
            }
        }
        __syncthreads();  // the previous chunk's LDS reads are done
        for (int e = tid; e < KC * CT / VW; e += 256) {
            const int kr = e / (CT / VW), cv = (e % (CT / VW)) * VW;
            V v;
            if (kc + kr < LP && c0 + cv < LP) {
                v = *reinterpret_cast<const V*>(Mm + (int64_t)(kc + kr) * LP + c0 + cv);
            } else {
                T* x = reinterpret_cast<T*>(&v);
#pragma unroll
                for (int t = 0; t < VW; ++t) x[t] = T(0);
            }
            *reinterpret_cast<V*>(Ms + kr * MP + cv) = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int k0 = kc + 4 * VW * j;
            if (k0 >= kmax) break;
            const T* ae = reinterpret_cast<const T*>(&a[j]);
#pragma unroll
            for (int t = 0; t < VW; ++t) {
                const T* mrow = Ms + (4 * VW * j + VW * h + t) * MP + r;
#pragma unroll
                for (int g = 0; g < G; ++g) acc[g] = M::mma(ae[t], mrow[16 * g], acc[g]);
            }
        }
    }
    // epilogue.  D: col = r (output column), row = M::row(h, j) (output row within the wave's 16)
    if (ldo == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t orow = row0 + 16 * w + M::row(h, j);
                const int c = c0 + 16 * g + r;
                if (orow < rows && c < LP) {
                    const T v = (T)acc[g][j];
                    if (Out) Out[orow * LP + c] = v;  // null: only the bf16 hi / lo panels are wanted
                    if (hi) {
                        const bf16_t bh = f2bf((float)v);
                        hi[orow * LP + c] = bh;
                        if (lo) lo[orow * LP + c] = f2bf((float)v - bf2f(bh));
                    }
                }
            }
        return;
    }
    // column-major caller output: transpose through LDS, store column segments contiguously
    __syncthreads();
    T* Ts = Ms;  // [CT][64 + 1]  (fits: KC * MP >= CT * 65 is checked at launch)
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int j = 0; j < 4; ++j) Ts[(16 * g + r) * 65 + 16 * w + M::row(h, j)] = acc[g][j];
    __syncthreads();
    for (int e = tid; e < CT * 64; e += 256) {
        const int c = e / 64, lr = e % 64;
        if (c0 + c < cols && row0 + lr < rows) Out[row0 + lr + (int64_t)(c0 + c) * ldo] = Ts[c * 65 + lr];
    }
}

// ------------------------------------------------------------------------------------------------
// Out = In * M for fp32 panels on the bf16 MFMA (panel_split_kernel): the three-piece split of
// the Gram kernel on both operands (In = h + m + t per element in registers, M pre-split into
// transposed piece images Mt[x][c][k] by split_mat_kernel) and the six products hH, hM, mH, mM,
// hT, tH per 32-deep k-step -- each term exact in fp32, the fp32 accumulation as the fp32 MFMA's.
// Six bf16 MFMAs cost 6/16 of one fp32 MFMA of the same shape: the product becomes a read of In
// plus the writes.  Workgroup: 128 rows x 128 columns (4 waves x 32 rows, 8 column tiles), M's
// 32 x 128 piece chunk staged in LDS per k-step (double-buffered, 64-B columns, 16-B units
// swizzled by (c >> 1) & 3 as the Gram images), In's fragment (8 consecutive k of one row) loaded
// one k-step ahead.  Upper-triangular M: K stops at the block's last column.
__global__ void split_mat_kernel(const float* __restrict__ M, int LP, bf16_t* __restrict__ Mt) {
    // Mt[x][c][k] = piece x of M[k][c]
    const int64_t L2 = (int64_t)LP * LP;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < L2; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e / LP), k = (int)(e % LP);
        const float v = M[(int64_t)k * LP + c];
        const bf16_t bh = f2bf(v);
        const float rm = v - bf2f(bh);
        const bf16_t bm = f2bf(rm);
        Mt[e] = bh;
        Mt[L2 + e] = bm;
        Mt[2 * L2 + e] = f2bf(rm - bf2f(bm));
    }
}

// RT2 row tiles (16 rows each) per wave, CT output columns per workgroup: the workgroup covers
// 64 RT2 rows x CT columns.  M's next chunk is loaded into registers while the current one is
// multiplied and written to the free LDS buffer after the MFMAs; the first version loaded and
// wrote it in one place before the MFMAs, exposing the L2 latency every step, and transposed
// column-major outputs through LDS.  Same shape (RT2 = 2, CT = 128), same box: C5 m-side product
// 454 -> 318 us, n side 51 -> 31 us, C4 74 -> 59 us (C5 31.0 -> 30.1 ms, C3 7.90 -> 7.50 ms).
template <typename F, int... I>
__device__ __forceinline__ void qr_static_for_impl(F& f, std::integer_sequence<int, I...>) {
    (f(std::integral_constant<int, I>{}), ...);
}
template <int N, typename F>
__device__ __forceinline__ void qr_static_for(F& f) {
    qr_static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// PD: In's fragments come through a ring of PD register sets, PD - 1 k-steps ahead (round 5: one
// step ahead left an HBM round trip exposed in every step of the short LP = 128 products).  The
// loads are unpredicated so the waits count them: rows past `rows` read the last row again, which
// only reaches output rows that are never stored (an MFMA output row depends on its A row alone).
template <int RT2, int CT, int PD = 2>
__global__ __launch_bounds__(256, 2) void panel_split_kernel(const float* __restrict__ In, int64_t rows, int LP,
                                                          const bf16_t* __restrict__ Mt, int upper,
                                                          float* __restrict__ Out, int64_t ldo, int cols,
                                                          bf16_t* __restrict__ hi, bf16_t* __restrict__ lo, int ncb,
                                                          const int* __restrict__ pred) {
    if (pred && *pred == 0) return;
    constexpr int G = CT / 16, IMG = CT * 64, STEPB = 3 * IMG, WR = 64 * RT2, NU = 3 * CT / 64;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int r = lane & 15, h = lane >> 4;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int cb = bid % ncb;
    const int64_t row0 = (int64_t)(bid / ncb) * WR;
    const int c0 = cb * CT;
    const int kmax = upper ? ((c0 + CT < LP) ? c0 + CT : LP) : LP;
    const int nk = (kmax + 31) / 32;
    const int64_t L2 = (int64_t)LP * LP;
    f32x4 acc[RT2][G];
#pragma unroll
    for (int t = 0; t < RT2; ++t)
#pragma unroll
        for (int g = 0; g < G; ++g) acc[t][g] = f32x4{0.f, 0.f, 0.f, 0.f};
    // M chunk: 3 pieces x CT columns x 64 B = 12 CT 16-B units, NU per thread
    uint4 mreg[NU];
    auto loadM = [&](int ks) {
#pragma unroll
        for (int t = 0; t < NU; ++t) {
            const int u = tid + 256 * t;
            const int x = u / (4 * CT), rem = u % (4 * CT), c = rem >> 2, un = rem & 3;
            mreg[t] = make_uint4(0u, 0u, 0u, 0u);
            if (c0 + c < LP) mreg[t] = *reinterpret_cast<const uint4*>(Mt + x * L2 + (int64_t)(c0 + c) * LP + 32 * ks + 8 * un);
        }
    };
    auto writeM = [&](char* img) {
#pragma unroll
        for (int t = 0; t < NU; ++t) {
            const int u = tid + 256 * t;
            const int x = u / (4 * CT), rem = u % (4 * CT), c = rem >> 2, un = rem & 3;
            *reinterpret_cast<uint4*>(img + x * IMG + c * 64 + 16 * (un ^ ((c >> 1) & 3))) = mreg[t];
        }
    };
    // In's fragments (8 consecutive k of the lane's row per row tile), ring of PD sets
    float4 ab[PD][RT2][2];
    auto loadA = [&](int ks, float4 (&a)[RT2][2]) {
        const int k = 32 * (ks < nk ? ks : nk - 1) + 8 * h;
#pragma unroll
        for (int t = 0; t < RT2; ++t) {
            const int64_t row = row0 + 16 * RT2 * w + 16 * t + r;
            const float* src = In + (row < rows ? row : rows - 1) * LP + k;
            a[t][0] = *reinterpret_cast<const float4*>(src);
            a[t][1] = *reinterpret_cast<const float4*>(src + 4);
        }
    };
    const uint32_t lofs = (uint32_t)(r * 64 + 16 * (h ^ ((r >> 1) & 3)));
    if (nk > 0) {
#pragma unroll
        for (int j = 0; j < PD - 1; ++j) loadA(j, ab[j]);
        loadM(0);
        writeM(smem_raw);
    }
    auto step = [&](int ks, float4 (&cur)[RT2][2], float4 (&ahead)[RT2][2]) __attribute__((always_inline)) {
        const char* img = smem_raw + (ks & 1) * STEPB;
        __syncthreads();  // chunk ks written; the readers of chunk ks - 1 (the other buffer) are done
        const bool more = ks + 1 < nk;
        loadA(ks + PD - 1, ahead);
        if (more) loadM(ks + 1);
        // In fragments of this k-step: three pieces of 8 consecutive k of the lane's row, per row tile
        bf16x8s fa[RT2][3];
#pragma unroll
        for (int t = 0; t < RT2; ++t) {
            const float v[8] = {cur[t][0].x, cur[t][0].y, cur[t][0].z, cur[t][0].w,
                                cur[t][1].x, cur[t][1].y, cur[t][1].z, cur[t][1].w};
            uint32_t ph[4], pm[4], pt[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ph[j] = cvt_pk_bf16(v[2 * j], v[2 * j + 1]);
                const float ra = v[2 * j] - __uint_as_float(ph[j] << 16);
                const float rb = v[2 * j + 1] - __uint_as_float(ph[j] & 0xffff0000u);
                pm[j] = cvt_pk_bf16(ra, rb);
                pt[j] = cvt_pk_bf16(ra - __uint_as_float(pm[j] << 16), rb - __uint_as_float(pm[j] & 0xffff0000u));
            }
            fa[t][0] = __builtin_bit_cast(bf16x8s, make_uint4(ph[0], ph[1], ph[2], ph[3]));
            fa[t][1] = __builtin_bit_cast(bf16x8s, make_uint4(pm[0], pm[1], pm[2], pm[3]));
            fa[t][2] = __builtin_bit_cast(bf16x8s, make_uint4(pt[0], pt[1], pt[2], pt[3]));
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const char* base = img + g * 1024 + lofs;
            const bf16x8s bh = *reinterpret_cast<const bf16x8s*>(base);
            const bf16x8s bm = *reinterpret_cast<const bf16x8s*>(base + IMG);
            const bf16x8s bt = *reinterpret_cast<const bf16x8s*>(base + 2 * IMG);
#pragma unroll
            for (int t = 0; t < RT2; ++t) {
                f32x4 c = acc[t][g];
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t][2], bh, c, 0, 0, 0);  // smallest terms first
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t][0], bt, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t][1], bm, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t][1], bh, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t][0], bm, c, 0, 0, 0);
                acc[t][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[t][0], bh, c, 0, 0, 0);
            }
        }
        if (more) writeM(smem_raw + ((ks + 1) & 1) * STEPB);
    };
    // whole groups of PD steps (each set at a fixed position in the ring), then the rest
    int ks0 = 0;
    for (; ks0 + PD <= nk; ks0 += PD) {
        auto one = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            step(ks0 + j, ab[j], ab[(j + PD - 1) % PD]);
        };
        qr_static_for<PD>(one);
    }
    {
        auto one = [&](auto jc) {
            constexpr int j = decltype(jc)::value;
            if (ks0 + j < nk) step(ks0 + j, ab[j], ab[(j + PD - 1) % PD]);
        };
        qr_static_for<PD>(one);
    }
    // epilogue.  bf16 MFMA D: col = r (output column c0 + 16 g + r), row = 4 h + j within the 16-row tile.
    // Row-major outputs go through LDS, 64 rows at a time (in the M buffers): a lane then owns 8
    // consecutive columns of one row and stores them as 32 B of fp32 and 16 B each of hi / lo --
    // from the accumulators a lane's values sit in 4 different rows, i.e. 2-byte hi / lo stores.
    if (ldo == 0) {
        constexpr int TP = CT + 4;  // fp32 pitch of the staged rows
        static_assert(64 * TP * 4 <= 2 * STEPB, "epilogue tile fits the M buffers");
        float* Ts = reinterpret_cast<float*>(smem_raw);
#pragma unroll
        for (int ch = 0; ch < RT2; ++ch) {  // 64-row chunks of the 64 RT2-row tile
            __syncthreads();                // the M buffers / the previous chunk are free
#pragma unroll
            for (int t = 0; t < RT2; ++t) {
                const int rt = 16 * RT2 * w + 16 * t;  // this row tile's first row in the workgroup
                if (rt / 64 != ch) continue;
#pragma unroll
                for (int g = 0; g < G; ++g)
#pragma unroll
                    for (int j = 0; j < 4; ++j) Ts[(rt % 64 + 4 * h + j) * TP + 16 * g + r] = acc[t][g][j];
            }
            __syncthreads();
            for (int e = tid; e < 64 * (CT / 8); e += 256) {
                const int lr = e / (CT / 8), c8 = 8 * (e % (CT / 8));
                const int64_t orow = row0 + 64 * ch + lr;
                const int c = c0 + c8;
                if (orow >= rows || c >= LP) continue;
                const float4 v0 = *reinterpret_cast<const float4*>(Ts + lr * TP + c8);
                const float4 v1 = *reinterpret_cast<const float4*>(Ts + lr * TP + c8 + 4);
                if (Out) {
                    *reinterpret_cast<float4*>(Out + orow * LP + c) = v0;
                    *reinterpret_cast<float4*>(Out + orow * LP + c + 4) = v1;
                }
                if (hi) {
                    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
                    uint32_t ph[4], pl[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const bf16_t h0 = f2bf(v[2 * q]), h1 = f2bf(v[2 * q + 1]);
                        ph[q] = (uint32_t)h0 | ((uint32_t)h1 << 16);
                        pl[q] = (uint32_t)f2bf(v[2 * q] - bf2f(h0)) | ((uint32_t)f2bf(v[2 * q + 1] - bf2f(h1)) << 16);
                    }
                    *reinterpret_cast<uint4*>(hi + orow * LP + c) = make_uint4(ph[0], ph[1], ph[2], ph[3]);
                    if (lo) *reinterpret_cast<uint4*>(lo + orow * LP + c) = make_uint4(pl[0], pl[1], pl[2], pl[3]);
                }
            }
        }
        return;
    }
    // column-major caller output: a lane holds 4 consecutive rows of one column -- one 16-B store
    // when Out and ldo allow it (4 lanes then write 64 contiguous bytes of the column)
    const bool vec = ((reinterpret_cast<uintptr_t>(Out) | (uintptr_t)(ldo * 4)) & 15) == 0;
#pragma unroll
    for (int t = 0; t < RT2; ++t)
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int64_t orow = row0 + 16 * RT2 * w + 16 * t + 4 * h;
            const int c = c0 + 16 * g + r;
            if (c >= cols) continue;
            float* dst = Out + orow + (int64_t)c * ldo;
            if (vec && orow + 3 < rows) {
                *reinterpret_cast<f32x4*>(dst) = acc[t][g];
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (orow + j < rows) dst[j] = acc[t][g][j];
            }
        }
}

}  // namespace

// panel_split_kernel shape: 2 row tiles x 128 columns (4 x 128 runs at one wave per SIMD and loses
// the gain of its halved LDS reads, 4 x 64 ties with 2 x 128 in the bench: round 3)
template <typename T>
hipError_t launch_panel_gemm(const T* In, int64_t rows, int LP, const T* Mm, int upper, T* Out, int64_t ldo,
                             int cols, bf16_t* hi, bf16_t* lo, const int* pred, hipStream_t s, bf16_t* msplit,
                             bool msplit_ready) {
    if (!Mm || LP % 16 || (!Out && (ldo != 0 || !hi))) return hipErrorInvalidValue;
    const int64_t rb = (rows + 63) / 64;
    if constexpr (sizeof(T) == 4) {
        if (msplit && LP % 32 == 0 && LP >= 128) {  // the bf16-split product (panel_split_kernel)
            const int64_t L2 = (int64_t)LP * LP;
            if (!msplit_ready)  // (else the factor that wrote M's fp32 copy wrote its pieces too)
                hipLaunchKernelGGL(split_mat_kernel, dim3((unsigned)std::min<int64_t>((L2 + 255) / 256, 1024)), dim3(256),
                                   0, s, reinterpret_cast<const float*>(Mm), LP, msplit);
            auto split = [&](auto pdc) {
                constexpr int RT2 = 2, CT = 128, PD = decltype(pdc)::value;
                const int ncb = (LP + CT - 1) / CT;
                const int64_t rb2 = (rows + 64 * RT2 - 1) / (64 * RT2);
                hipLaunchKernelGGL((panel_split_kernel<RT2, CT, PD>), dim3((unsigned)(rb2 * ncb)), dim3(256),
                                   (size_t)2 * 3 * CT * 64, s, reinterpret_cast<const float*>(In), rows, LP, msplit,
                                   upper, reinterpret_cast<float*>(Out), ldo, cols, hi, lo, ncb, pred);
                return hipGetLastError();
            };
            // In prefetch ring depth (RSVD_PANEL_PD overrides): 4 at LP = 512 (16 k-steps: C5 18.38 ->
            // 18.19 ms, gpurun_out r6k), 2 (one step ahead) below, where 3 / 4 measured no gain
            static const int pd_env = [] {
                const char* e = std::getenv("RSVD_PANEL_PD");
                return e ? std::atoi(e) : 0;
            }();
            const int pd = pd_env ? pd_env : (LP >= 512 ? 4 : 2);
            if (pd == 3) return split(std::integral_constant<int, 3>{});
            if (pd == 4) return split(std::integral_constant<int, 4>{});
            return split(std::integral_constant<int, 2>{});
        }
    }
    auto go = [&](auto ctc) {
        constexpr int CT = decltype(ctc)::value;
        const int ncb = (LP + CT - 1) / CT;
        constexpr int KC = 16 * PG<T>::VW;
        const size_t lds = std::max<size_t>((size_t)KC * (CT + PG<T>::PAD), (size_t)CT * 65) * sizeof(T);
        hipLaunchKernelGGL((panel_gemm_kernel<T, CT>), dim3((unsigned)(rb * ncb)), dim3(256), lds, s, In, rows, LP, Mm,
                           upper, Out, ldo, cols, hi, lo, ncb, pred);
        return hipGetLastError();
    };
    if (LP <= 16) return go(std::integral_constant<int, 16>{});
    if (LP <= 32) return go(std::integral_constant<int, 32>{});
    if (LP <= 64) return go(std::integral_constant<int, 64>{});
    return go(std::integral_constant<int, 128>{});
}

namespace {

// ------------------------------------------------------------------------------------------------
// Elementwise kernels of the host pipeline.
template <typename T>
__global__ void repair_kernel(const T* __restrict__ Q, int64_t rows, int l, int LP, const int* __restrict__ colflag,
                              const int* __restrict__ flag, uint64_t seed, int64_t row_off, int64_t rows_total,
                              int64_t norm_rows, int64_t valid_rows, T* __restrict__ Out) {
    if (*flag == 0) return;
    const double sc = 1.0 / sqrt((double)norm_rows);
    const int64_t total = rows * LP;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / LP;
        const int c = (int)(e - i * LP);
        T v = Q[e];
        if (c < l && colflag[c])  // (rows past valid_rows: the zero padding of a sharded panel stays zero)
            v = i < valid_rows ? (T)(gauss_elem((uint64_t)(row_off + i + rows_total * (int64_t)c), seed) * sc) : (T)0;
        Out[e] = v;
    }
}

template <typename T>
__global__ void split_bf16_kernel(const T* __restrict__ P, int64_t count, bf16_t* __restrict__ hi,
                                  bf16_t* __restrict__ lo) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count; e += (int64_t)gridDim.x * blockDim.x) {
        const float v = (float)P[e];
        const bf16_t bh = f2bf(v);
        hi[e] = bh;
        if (lo) lo[e] = f2bf(v - bf2f(bh));
    }
}

// Round x to `bits` significant bits (round half to even), e4m3: saturate at 448 and keep the
// subnormal quantum 2^-9.  Mirrored bit for bit by the oracle's Python front end.
__device__ __forceinline__ double round_sig(double x, int fp8) {
    if (x == 0.0 || !isfinite(x)) return x;
    int e;
    (void)frexp(x, &e);  // |x| = m 2^e, m in [0.5, 1)
    int ex = e - 1;      // floor(log2 |x|)
    int bits = fp8 ? 3 : 7;
    if (fp8 && ex < -6) ex = -6;
    const double qn = ldexp(1.0, ex - bits);
    double y = rint(x / qn) * qn;
    if (fp8) y = fmin(fmax(y, -448.0), 448.0);
    return y;
}

// One thread per PAIR of stream elements (e, e + 1) = rows (i, i + 1) of column c (n even, i even):
// the two share the Philox block, log and square root of gauss_elem -- the same operations, so the
// values are bit-identical to gauss_elem's (cos for the even element, sin for the odd one); an odd n
// falls back to one element per thread.  C4's 65536 x 256 Omega: half the Philox / log / sqrt work.
__device__ __forceinline__ void gauss_pair(uint64_t e, uint64_t seed, double& g0, double& g1) {
    uint32_t x[4];
    philox4x32_10(e >> 1, seed, x);
    const double two_m53 = 1.1102230246251565404e-16;
    const double u1 = ((double)(((uint64_t)(x[0] >> 5) << 26) | (x[1] >> 6)) + 0.5) * two_m53;
    const double u2 = ((double)(((uint64_t)(x[2] >> 5) << 26) | (x[3] >> 6)) + 0.5) * two_m53;
    const double rr = sqrt(-2.0 * log(u1));
    const double th = 6.283185307179586476925286766559 * u2;
    g0 = rr * cos(th);
    g1 = rr * sin(th);
}

__global__ void omega_lowp_kernel(bf16_t* __restrict__ panel, int64_t n, int l, int LP, uint64_t seed, int fp8,
                                  float* __restrict__ f) {
    if ((n & 1) == 0) {
        const int64_t total = (n >> 1) * LP;  // (row pair, column)
        for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
             e += (int64_t)gridDim.x * blockDim.x) {
            const int64_t i = 2 * (e / LP);
            const int c = (int)(e % LP);
            float v0 = 0.f, v1 = 0.f;
            if (c < l) {
                double g0, g1;
                gauss_pair((uint64_t)(i + n * (int64_t)c), seed, g0, g1);  // even stream index
                v0 = (float)round_sig(g0, fp8);
                v1 = (float)round_sig(g1, fp8);
                if (f) {
                    f[i + n * (int64_t)c] = v0;
                    f[i + 1 + n * (int64_t)c] = v1;
                }
            }
            panel[i * LP + c] = (bf16_t)(__float_as_uint(v0) >> 16);  // exact: <= 8 significant bits
            panel[(i + 1) * LP + c] = (bf16_t)(__float_as_uint(v1) >> 16);
        }
        return;
    }
    const int64_t total = n * LP;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / LP;
        const int c = (int)(e - i * LP);
        float v = 0.f;
        if (c < l) {
            v = (float)round_sig(gauss_elem((uint64_t)(i + n * (int64_t)c), seed), fp8);
            if (f) f[i + n * (int64_t)c] = v;
        }
        panel[e] = (bf16_t)(__float_as_uint(v) >> 16);  // exact: v has <= 8 significant bits
    }
}

__global__ void omega_lowp_from_kernel(const float* __restrict__ om, int64_t ld, int64_t n, int l, int LP, int fp8,
                                       bf16_t* __restrict__ panel) {
    const int64_t total = n * LP;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = e / LP;
        const int c = (int)(e - i * LP);
        const float v = (c < l) ? (float)round_sig((double)om[i + ld * c], fp8) : 0.f;
        panel[e] = (bf16_t)(__float_as_uint(v) >> 16);
    }
}

// bf16 values that are exactly e4m3 -> e4m3 codes, 4 per thread (exact: no rounding happens)
__global__ void bf16_to_fp8_kernel(const bf16_t* __restrict__ in, int64_t count4, uint32_t* __restrict__ out) {
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < count4; e += (int64_t)gridDim.x * blockDim.x) {
        const uint2 v = reinterpret_cast<const uint2*>(in)[e];
        const float f0 = __uint_as_float(v.x << 16), f1 = __uint_as_float(v.x & 0xFFFF0000u);
        const float f2 = __uint_as_float(v.y << 16), f3 = __uint_as_float(v.y & 0xFFFF0000u);
        int w = __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, 0, false);
        w = __builtin_amdgcn_cvt_pk_fp8_f32(f2, f3, w, true);
        out[e] = (uint32_t)w;
    }
}

template <typename T>
__global__ void convert_scale_kernel(const double* __restrict__ x, T* __restrict__ y, int n, double sc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = (T)(x[i] * sc);
}

// The small SVD's outputs for the fp32 final products in one launch: S (scaled), U_w and V_w in fp32
// and, for the split panel products, their bf16 piece images (split_mat_kernel's layout)
__global__ void finish_convert_kernel(const double* __restrict__ Sd, float* __restrict__ S, int l, double sc,
                                      const double* __restrict__ Uw, float* __restrict__ Uw32, bf16_t* __restrict__ Mu,
                                      const double* __restrict__ Vw, float* __restrict__ Vw32, bf16_t* __restrict__ Mv,
                                      int LP) {
    const int64_t L2 = (int64_t)LP * LP;
    for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < L2; e += (int64_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / LP), c = (int)(e - (int64_t)k * LP);
        const int64_t t = (int64_t)c * LP + k;
        const float u = (float)Uw[e], v = (float)Vw[e];
        Uw32[e] = u;
        Vw32[e] = v;
        store_pieces(Mu, L2, t, u);
        store_pieces(Mv, L2, t, v);
        if (e < l) S[e] = (float)(Sd[e] * sc);
    }
}

inline int grid_1d(int64_t work) {
    int64_t g = (work + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

}  // namespace

template <typename T>
hipError_t launch_repair_panel(const T* Q, int64_t rows, int l, int LP, const int* colflag, const int* flag,
                               uint64_t seed, int64_t row_off, int64_t rows_total, int64_t norm_rows, T* Out,
                               hipStream_t s, int64_t valid_rows) {
    hipLaunchKernelGGL((repair_kernel<T>), dim3(grid_1d(rows * LP)), dim3(256), 0, s, Q, rows, l, LP, colflag, flag,
                       seed, row_off, rows_total, norm_rows, valid_rows < 0 ? rows : valid_rows, Out);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_split_bf16(const T* P, int64_t rows, int LP, bf16_t* hi, bf16_t* lo, hipStream_t s) {
    hipLaunchKernelGGL((split_bf16_kernel<T>), dim3(grid_1d(rows * LP)), dim3(256), 0, s, P, rows * LP, hi, lo);
    return hipGetLastError();
}

hipError_t launch_omega_lowp(bf16_t* panel, int64_t n, int l, int LP, uint64_t seed, int round_fp8, float* f,
                             hipStream_t s) {
    hipLaunchKernelGGL(omega_lowp_kernel, dim3(grid_1d(n * LP)), dim3(256), 0, s, panel, n, l, LP, seed, round_fp8,
                       f);
    return hipGetLastError();
}

hipError_t launch_bf16_to_fp8(const bf16_t* in, int64_t count, fp8_t* out, hipStream_t s) {
    if (count % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bf16_to_fp8_kernel, dim3(grid_1d(count / 4)), dim3(256), 0, s, in, count / 4,
                       reinterpret_cast<uint32_t*>(out));
    return hipGetLastError();
}

hipError_t launch_omega_lowp_from(const float* om, int64_t ld, int64_t n, int l, int LP, int round_fp8,
                                  bf16_t* panel, hipStream_t s) {
    hipLaunchKernelGGL(omega_lowp_from_kernel, dim3(grid_1d(n * LP)), dim3(256), 0, s, om, ld, n, l, LP, round_fp8,
                       panel);
    return hipGetLastError();
}

hipError_t launch_finish_convert(const double* Sd, float* S, int l, double sc, const double* Uw, float* Uw32, bf16_t* Mu,
                                 const double* Vw, float* Vw32, bf16_t* Mv, int LP, hipStream_t s) {
    const int64_t L2 = (int64_t)LP * LP;
    hipLaunchKernelGGL(finish_convert_kernel, dim3((unsigned)std::min<int64_t>((L2 + 255) / 256, 1024)), dim3(256), 0, s,
                       Sd, S, l, sc, Uw, Uw32, Mu, Vw, Vw32, Mv, LP);
    return hipGetLastError();
}

template <typename T>
hipError_t launch_convert_scale(const double* x, T* y, int n, double sc, hipStream_t s) {
    hipLaunchKernelGGL((convert_scale_kernel<T>), dim3((n + 255) / 256), dim3(256), 0, s, x, y, n, sc);
    return hipGetLastError();
}

#define RSVD_INST(T)                                                                                              \
    template hipError_t launch_convert_scale<T>(const double*, T*, int, double, hipStream_t);                     \
    template hipError_t launch_panel_gemm<T>(const T*, int64_t, int, const T*, int, T*, int64_t, int, bf16_t*,    \
                                             bf16_t*, const int*, hipStream_t, bf16_t*, bool);                    \
    template hipError_t launch_repair_panel<T>(const T*, int64_t, int, int, const int*, const int*, uint64_t,     \
                                               int64_t, int64_t, int64_t, T*, hipStream_t, int64_t);              \
    template hipError_t launch_split_bf16<T>(const T*, int64_t, int, bf16_t*, bf16_t*, hipStream_t);
RSVD_INST(float)
RSVD_INST(double)
#undef RSVD_INST

}  // namespace rsvd
