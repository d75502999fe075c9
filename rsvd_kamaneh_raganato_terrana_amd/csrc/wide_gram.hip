// wide_gram.hip -- G = P^T P (and the cross Gram X^T Y) of the wide engine's CholeskyQR (wide.hpp): the
// fp64-MFMA Grams, the three-piece bf16 split Grams and the fixed-order chunk reduction they all end in.
#include <type_traits>
#include <utility>

#include "wide_dev.hpp"

namespace rsvd {

namespace {

constexpr bool gram_sym_ok(int LP) { return LP == 64 || LP == 128 || LP == 256 || LP == 512; }

template <typename T> struct Pair;
template <> struct Pair<float> { typedef float2 type; };
template <> struct Pair<double> { typedef double2 type; };

// The chunk partials summed in a fixed order (deterministic): one workgroup = 64 Gram entries x 4
// chunk ranges (wave k sums chunks [k n / 4, (k + 1) n / 4) with four interleaved partials, a wave's
// 64 entries one 512-B load per chunk), the ranges combined in wave order.  (Round 4 replaced a
// one-thread-per-entry sum: C3's LP = 128 Gram -- 10 blocks, 256 chunks -- ran that on 40 workgroups;
// this gives it 160: C4 23.81 -> 23.68 ms, C5 19.15 -> 19.13, C3 5.65 -> 5.62 on one box.)
__global__ __launch_bounds__(256) void gram_reduce4_kernel(const double* __restrict__ slabs, int nblk, int nchunk,
                                                           int LP, int cross, double* __restrict__ G,
                                                           const int* __restrict__ pred) {
    if (pred && *pred == 0) return;
    __shared__ double part[4][64];
    const int lane = threadIdx.x & 63, k = threadIdx.x >> 6;
    const int64_t e = blockIdx.x * (int64_t)64 + lane;
    bool ok = e < (int64_t)nblk * 1024;
    const int blk = ok ? (int)(e / 1024) : 0, loc = (int)(e % 1024);
    const int nb = (LP + 31) / 32;
    int a, b;
    if (cross) {
        a = blk / nb;
        b = blk % nb;
    } else {
        int rem = blk;
        a = 0;
        while (rem >= nb - a) {
            rem -= nb - a;
            ++a;
        }
        b = a + rem;
    }
    const int ra = 32 * a + loc / 32, cb = 32 * b + loc % 32;
    ok = ok && ra < LP && cb < LP;
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
        const double t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        G[(int64_t)ra * LP + cb] = t;
        if (!cross && a != b) G[(int64_t)cb * LP + ra] = t;
    }
}

hipError_t launch_gram_reduce(const double* slabs, int nblk, int nchunk, int LP, int cross, double* G, const int* pred,
                              hipStream_t s) {
    const int64_t tot = (int64_t)nblk * 1024;
    hipLaunchKernelGGL(gram_reduce4_kernel, dim3((int)((tot + 63) / 64)), dim3(256), 0, s, slabs, nblk, nchunk, LP,
                       cross, G, pred);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Gram: one wave per (32x32 block, row chunk).  Tile (ta, tb) of the block holds columns
// a0 + 2i + ta (i = MFMA row) and b0 + 2j + tb (j = MFMA col): each lane's 2-element vector load
// feeds both tiles of its side.
template <typename T, bool CROSS>
__global__ __launch_bounds__(256) void gram_wide_kernel(const T* __restrict__ P, const T* __restrict__ P2,
                                                        int64_t rows, int LP, int nblk, int nchunk, int64_t rpc,
                                                        double* __restrict__ slabs, const int* __restrict__ pred) {
    if (pred && *pred == 0) return;
    typedef typename Pair<T>::type V2;
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int blk = gw % nblk, chunk = gw / nblk;
    if (chunk >= nchunk) return;
    const int nb = (LP + 31) / 32;
    int a, b;
    if (CROSS) {
        a = blk / nb;
        b = blk % nb;
    } else {
        int rem = blk;
        a = 0;
        while (rem >= nb - a) {
            rem -= nb - a;
            ++a;
        }
        b = a + rem;
    }
    const int r = lane & 15, h = lane >> 4;
    const int ca = 32 * a + 2 * r, cb = 32 * b + 2 * r;
    const bool oka = ca < LP, okb = cb < LP;  // LP is a multiple of 16: pairs never straddle it
    const int64_t beg = (int64_t)chunk * rpc;
    const int64_t end = (beg + rpc < rows) ? beg + rpc : rows;
    f64x4 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = MD::zero();
    for (int64_t i0 = beg; i0 < end; i0 += 16) {
        V2 va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t row = i0 + 4 * u + h;
            va[u].x = va[u].y = vb[u].x = vb[u].y = T(0);
            if (row < end) {
                if (oka) va[u] = *reinterpret_cast<const V2*>(P + row * LP + ca);
                if (okb) vb[u] = *reinterpret_cast<const V2*>((CROSS ? P2 : P) + row * LP + cb);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double a0 = (double)va[u].x, a1 = (double)va[u].y;
            const double b0 = (double)vb[u].x, b1 = (double)vb[u].y;
            acc[0][0] = MD::mma(a0, b0, acc[0][0]);
            acc[0][1] = MD::mma(a0, b1, acc[0][1]);
            acc[1][0] = MD::mma(a1, b0, acc[1][0]);
            acc[1][1] = MD::mma(a1, b1, acc[1][1]);
        }
    }
    double* dst = slabs + ((int64_t)chunk * nblk + blk) * 1024;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = MD::row(h, j);
                dst[(2 * i + x) * 32 + 2 * r + y] = acc[x][y][j];
            }
}

// ------------------------------------------------------------------------------------------------
// Symmetric Gram of a tall panel, LP in {64, 128, 256}: ONE 512-thread workgroup per row chunk reads
// its rows once (16-B loads, register-prefetched one step ahead, staged in LDS 32 rows per step) and
// computes every upper 16x16 tile pair (ta <= tb) of the chunk on the fp64 MFMA (LP = 256: two workgroups per chunk).  For G = P^T P both
// MFMA operands are "row k, column c" reads of the panel (A: P^T[c][k], B: P[k][c]), so a tile pair
// costs two LDS reads per 4 rows.  Pairs are dealt round-robin to the waves (9 per wave at
// LP = 256).  The old kernel gave each 32x32 block its own wave and chunk walk, re-reading every
// panel row LP/32 + 1 times from HBM; here each byte is read once and the MFMA issue rate is the
// bound.  Partial tiles land in the (chunk, 32x32 block) slab layout gram_reduce4_kernel sums; the
// lower 16x16 sub-tile of a diagonal 32x32 block is written as the transpose of the upper one.
// (ta, tb) of upper tile pair p (row-major over the upper triangle of NT x NT tiles); p >= NP -> (0, 0)
constexpr int pair_ta(int NT, int p) {
    if (p >= NT * (NT + 1) / 2) return 0;
    int a = 0;
    while (p >= NT - a) { p -= NT - a; ++a; }
    return a;
}
constexpr int pair_tb(int NT, int p) {
    if (p >= NT * (NT + 1) / 2) return 0;
    int a = 0;
    while (p >= NT - a) { p -= NT - a; ++a; }
    return a + p;
}

template <int NT, int P> struct PairOf {  // forces compile-time evaluation of the tile indices
    static constexpr int a = pair_ta(NT, P), b = pair_tb(NT, P);
};

template <int LP> struct GramSym {
    static constexpr int NH = LP == 512 ? 8 : (LP == 256 ? 2 : 1);  // workgroups per chunk
    static constexpr int LNH = LP == 512 ? 3 : (LP == 256 ? 1 : 0);
    // panel rows per LDS step (static LDS <= 64 KB)
    template <typename T> static constexpr int rs() { return LP == 512 ? (sizeof(T) == 8 ? 8 : 16) : ((sizeof(T) == 8 && LP == 256) ? 16 : 32); }
    static constexpr int NT = LP / 16, NP = NT * (NT + 1) / 2, NW = 8 * NH, PPW = (NP + NW - 1) / NW;
    static constexpr int NB = LP / 32, NBLK = NB * (NB + 1) / 2;
};

// slot I of dealer WG: pair WG + NW I (compile-time tile indices, so v[] stays in registers)
template <int LP, int WG, int... I>
__device__ __forceinline__ void gram_sym_mma(const double (&v)[LP / 16], f64x4 (&acc)[GramSym<LP>::PPW],
                                             std::integer_sequence<int, I...>) {
    typedef GramSym<LP> G;
    ((acc[I] = (WG + G::NW * I < G::NP) ? MD::mma(v[PairOf<G::NT, WG + G::NW * I>::a], v[PairOf<G::NT, WG + G::NW * I>::b], acc[I])
                                        : acc[I]),
     ...);
}

// does dealer WG touch tile t?
template <int LP, int WG>
constexpr bool gram_sym_needs(int t) {
    typedef GramSym<LP> G;
    for (int i = 0; i < G::PPW; ++i)
        if (WG + G::NW * i < G::NP && (pair_ta(G::NT, WG + G::NW * i) == t || pair_tb(G::NT, WG + G::NW * i) == t))
            return true;
    return false;
}

template <int LP, int WG, int t> struct NeedOf {  // compile-time gram_sym_needs
    static constexpr bool value = gram_sym_needs<LP, WG>(t);
};
// the panel values of the tiles dealer WG touches, for the 4 rows of one MFMA step
template <typename T, int LP, int WG, int... I>
__device__ __forceinline__ void gram_sym_loadv(const T* rowp, double (&v)[LP / 16], std::integer_sequence<int, I...>) {
    ((v[I] = NeedOf<LP, WG, I>::value ? (double)rowp[16 * I] : 0.0), ...);
}

template <typename T, int LP, int WG>
__device__ __forceinline__ void gram_sym_body(const T* __restrict__ P, int64_t beg, int64_t end, int chunk,
                                              double* __restrict__ slabs, T* tile) {
    typedef GramSym<LP> G;
    constexpr int NT = G::NT, PPW = G::PPW, NTH = 512;
    constexpr int RS = G::template rs<T>();  // panel rows per step
    constexpr int VE = 16 / sizeof(T);                            // elements per 16-B load
    constexpr int CPR = LP / VE;                                  // 16-B chunks per row
    constexpr int LPT = RS * CPR / NTH;                           // loads per thread per step
    static_assert(LPT >= 1 && (RS * CPR) % NTH == 0, "step tiling");
    constexpr int PITCH = LP + 64 / (int)sizeof(T);  // row pitch: the 4 rows of an MFMA read hit different banks
    typedef typename Vec16<T>::type V;
    const int tid = threadIdx.x, lane = tid & 63;
    const int r = lane & 15, h = lane >> 4;
    f64x4 acc[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) acc[i] = MD::zero();

    V reg[LPT];
    auto load = [&](int64_t r0) {
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            const int u = tid + NTH * t;
            const int64_t row = r0 + u / CPR;
            V v;
            if constexpr (sizeof(T) == 4) v = make_float4(0.f, 0.f, 0.f, 0.f);
            else v = make_double2(0.0, 0.0);
            if (row < end) v = *reinterpret_cast<const V*>(P + row * LP + (u % CPR) * VE);
            reg[t] = v;
        }
    };
    if (beg < end) load(beg);
    for (int64_t r0 = beg; r0 < end; r0 += RS) {
        __syncthreads();  // the previous step's LDS reads are done
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            const int u = tid + NTH * t;
            *reinterpret_cast<V*>(tile + (u / CPR) * PITCH + (u % CPR) * VE) = reg[t];
        }
        __syncthreads();
        if (r0 + RS < end) load(r0 + RS);
#pragma unroll 2
        for (int g = 0; g < RS / 4; ++g) {
            const T* rowp = tile + (4 * g + h) * PITCH + r;
            double v[NT];
            gram_sym_loadv<T, LP, WG>(rowp, v, std::make_integer_sequence<int, NT>{});
            gram_sym_mma<LP, WG>(v, acc, std::make_integer_sequence<int, PPW>{});
        }
    }

#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int p = WG + G::NW * i;
        if (p < G::NP) {
            const int ta = pair_ta(NT, p), tb = pair_tb(NT, p);
            const int a = ta >> 1, b = tb >> 1;
            const int blk = a * G::NB - a * (a - 1) / 2 + (b - a);
            double* dst = slabs + ((int64_t)chunk * G::NBLK + blk) * 1024;
            const bool mirror = (a == b) && (ta != tb);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int li = 16 * (ta & 1) + MD::row(h, j), lj = 16 * (tb & 1) + r;
                dst[li * 32 + lj] = acc[i][j];
                if (mirror) dst[lj * 32 + li] = acc[i][j];
            }
        }
    }
}

template <typename T, int LP, int... W>
__device__ __forceinline__ void gram_sym_dispatch(int wg, const T* P, int64_t beg, int64_t end, int chunk, double* slabs,
                                                  T* tile, std::integer_sequence<int, W...>) {
    ((wg == W ? gram_sym_body<T, LP, W>(P, beg, end, chunk, slabs, tile) : void()), ...);
}

template <typename T, int LP>
__global__ __launch_bounds__(512) void gram_sym_kernel(const T* __restrict__ P, int64_t rows, int64_t rpc, int nchunk,
                                                       double* __restrict__ slabs, const int* __restrict__ pred) {
    if (pred && *pred == 0) return;
    typedef GramSym<LP> G;
    // NH workgroups share a chunk (LP = 256: 2, LP = 512: 8, dealing the pairs between them), all on one
    // XCD (block ids b, b + 8, ...) so the repeated reads of the rows are L2 hits.
    constexpr int RS = G::template rs<T>();
    constexpr int PITCH = LP + 64 / (int)sizeof(T);
    __shared__ __attribute__((aligned(16))) T tile[RS * PITCH];
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: scalar branch to the dealer body
    const int hb = G::NH == 1 ? 0 : (blockIdx.x >> 3) & (G::NH - 1);
    const int chunk = G::NH == 1 ? blockIdx.x : ((blockIdx.x & 7) | ((blockIdx.x >> (3 + G::LNH)) << 3));
    if (chunk >= nchunk) return;
    const int64_t beg = (int64_t)chunk * rpc;
    const int64_t end = (beg + rpc < rows) ? beg + rpc : rows;
    // dealer index: pairs WG, WG + NW, ... belong to wave w of half hb
    gram_sym_dispatch<T, LP>(w * G::NH + hb, P, beg, end, chunk, slabs, tile, std::make_integer_sequence<int, G::NW>{});
}

}  // namespace

GramPlan plan_gram_wide(int64_t rows, int LP, int cross) {
    GramPlan g;
    const int nb = (LP + 31) / 32;
    g.blocks = cross ? nb * nb : nb * (nb + 1) / 2;
    if (!cross && gram_sym_ok(LP)) {  // gram_sym_kernel: one workgroup per chunk, >= 64 rows each, <= 256 chunks
        // >= max(64, LP) rows per chunk: a chunk's slab (LP^2 / 2 doubles) must not outweigh its rows
        const int64_t rmin = LP > 64 ? LP : 64;
        int64_t chunks = (rows + rmin - 1) / rmin;
        const int64_t cap = LP == 512 ? 128 : 256;  // LP = 512: 8 workgroups per chunk, 1 MB of slab per chunk
        if (chunks > cap) chunks = cap;
        if (chunks < 1) chunks = 1;
        int64_t rpc = (rows + chunks - 1) / chunks;
        rpc = (rpc + 31) / 32 * 32;  // a multiple of every RS
        g.rows_per_chunk = rpc;
        g.chunks = (int)((rows + rpc - 1) / rpc);
        if (g.chunks < 1) g.chunks = 1;
        return g;
    }
    int64_t chunks = (4096 + g.blocks - 1) / g.blocks;
    const int64_t max_by_rows = (rows + 255) / 256;
    if (chunks > max_by_rows) chunks = max_by_rows;
    if (chunks > 512) chunks = 512;
    if (chunks < 1) chunks = 1;
    int64_t rpc = (rows + chunks - 1) / chunks;
    rpc = (rpc + 15) / 16 * 16;
    g.rows_per_chunk = rpc;
    g.chunks = (int)((rows + rpc - 1) / rpc);
    if (g.chunks < 1) g.chunks = 1;
    return g;
}

template <typename T>
hipError_t launch_gram_wide(const T* P, const T* P2, int64_t rows, int LP, const GramPlan& gp, double* slabs,
                            double* G, const int* pred, hipStream_t s) {
    const int waves = gp.blocks * gp.chunks;
    const int wgs = (waves + 3) / 4;
    if (P2)
        hipLaunchKernelGGL((gram_wide_kernel<T, true>), dim3(wgs), dim3(256), 0, s, P, P2, rows, LP, gp.blocks,
                           gp.chunks, gp.rows_per_chunk, slabs, pred);
    else if (gram_sym_ok(LP)) {
        auto go = [&](auto lpc) {
            constexpr int L = decltype(lpc)::value;
            const int grid = GramSym<L>::NH == 1 ? gp.chunks : (gp.chunks + 7) / 8 * 8 * GramSym<L>::NH;
            hipLaunchKernelGGL((gram_sym_kernel<T, L>), dim3(grid), dim3(512), 0, s, P, rows, gp.rows_per_chunk,
                               gp.chunks, slabs, pred);
        };
        if (LP == 64) go(std::integral_constant<int, 64>{});
        else if (LP == 128) go(std::integral_constant<int, 128>{});
        else if (LP == 256) go(std::integral_constant<int, 256>{});
        else go(std::integral_constant<int, 512>{});
    } else
        hipLaunchKernelGGL((gram_wide_kernel<T, false>), dim3(wgs), dim3(256), 0, s, P, P, rows, LP, gp.blocks,
                           gp.chunks, gp.rows_per_chunk, slabs, pred);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_gram_reduce(slabs, gp.blocks, gp.chunks, LP, P2 ? 1 : 0, G, pred, s);
}

template hipError_t launch_gram_wide<float>(const float*, const float*, int64_t, int, const GramPlan&, double*, double*,
                                            const int*, hipStream_t);
template hipError_t launch_gram_wide<double>(const double*, const double*, int64_t, int, const GramPlan&, double*,
                                             double*, const int*, hipStream_t);

namespace {

// ------------------------------------------------------------------------------------------------
// Split Gram of an fp32 panel on the bf16 MFMA.  Every fp32 value is EXACTLY h + m + t with
// h = bf16(v), m = bf16(v - h), t = bf16(v - h - m) (8 + 8 + 8 significant bits), and the six
// products hh, hm, mh, mm, ht, th carry P_ki P_kj to ~2^-24 of |P_ki P_kj| (the dropped mt, tm,
// tt are below it).  Each bf16 product is exact in fp32; the v_mfma_f32_16x16x32_bf16 chains sum a
// row chunk (<= 1024 rows at the configs' sizes) in fp32 and the chunk partials are summed in fp64,
// so the rounding does not grow with the panel height: numpy model of the same arithmetic on a
// cond 1e3 panel (65536 x 256): |G_split - G|_F / |G|_F ~ 1e-8, max |dG_ij| / sqrt(G_ii G_jj) ~ 3e-8.  Six bf16 MFMAs at 32x the fp64 MFMA rate: the Gram becomes an HBM read of the panel
// (C4 65536 x 256: ~100 -> ~20 us).  It is only used where its accuracy is enough -- CholeskyQR of
// the fp32 panels of bf16 / e4m3 A, with the factor's pivots checked against kSplitIllTol
// (launch_chol, CholArgs::ill) and the fp64 Gram + factor re-run (predicated) when one is below it.
// Layout: a 32-row step is staged as three [LP column][32 row] bf16 images (64-B columns, 16-B
// unit u of column c at u ^ ((c >> 1) & 3): the 16-lane ds_read_b128 of one tile is conflict-free);
// lane (r, h) of tile t reads rows 8h .. 8h + 7 of column 16t + r -- the A and the B fragment of
// v_mfma_f32_16x16x32_bf16 alike (G = P^T P: both operands are "column, rows k" reads).
// Upper tile pairs (ta <= tb) are dealt to the NH x 8 waves of a chunk at compile time; the
// partial tiles go to gram_sym's (chunk, 32x32 block) slab layout, summed by gram_reduce4_kernel.

// Work split: the tiles are cut into groups of TG (4; 2 at LP = 128) and each wave owns one
// group pair (A <= B) -- TG x TG tile pairs whose A-side fragments stay in registers for the step
// while the B-side ones stream (each fragment feeds TG x 6 MFMAs: ~0.25 KB of LDS reads per MFMA;
// one fragment pair per tile pair read 1 KB per MFMA and made the kernel LDS-bound).  Diagonal
// group pairs compute their TG^2 tile pairs in full and store the upper ones.  The fp32 MFMA
// accumulators run over the whole row chunk (<= 1024 rows for the panels of the bf16 / e4m3
// configs) and the chunk partials are summed in fp64 by gram_reduce4_kernel.
template <int LP> struct GramSplit {
    static constexpr int TG = LP == 128 ? 2 : 4;
    static constexpr int NT = LP / 16, NTG = NT / TG, NBK = NTG * (NTG + 1) / 2;
    static constexpr int NH = LP == 512 ? 4 : 1;  // workgroups per chunk
    static constexpr int LNH = LP == 512 ? 2 : 0;
    static constexpr int NWW = NBK / NH;          // waves per workgroup (10, 10, 9)
    static constexpr int THREADS = 64 * NWW;
    static constexpr int NB = LP / 32, NBLK = NB * (NB + 1) / 2;
    static constexpr int IMG = LP * 64;           // bytes of one piece image (LP columns x 32 rows bf16)
    static constexpr int STEP = 3 * IMG;          // the three pieces of a 32-row step
    static constexpr int NBUF = STEP * 2 <= 98304 ? 2 : 1;
    static constexpr int NU = 2 * LP;             // 4-row x 4-column units of a 32-row step
    static constexpr int LPT = (NU + THREADS - 1) / THREADS;
    static_assert(NBK % NH == 0, "group pairs per workgroup");
};

// Loader groups (round 4): the NU units of a step are loaded by GSZ = NU / LPTG threads, LPTG units
// each; NLG such groups take the steps round robin, so a group issues its next load NLG steps ahead
// of the step it stages.  <1, 1> is the original one-step prefetch; at LP = 128 one step is 16 KB per
// CU and the 1-step prefetch left the kernel waiting on HBM latency (205 us for a 2^20-row panel).
template <int LP, int LPTG = GramSplit<LP>::LPT, int NLG = 1>
__global__ __launch_bounds__(GramSplit<LP>::THREADS) void gram_split_kernel(const float* __restrict__ P, int64_t rows,
                                                                          int64_t rpc, int nchunk,
                                                                          double* __restrict__ slabs) {
    typedef GramSplit<LP> G;
    constexpr int TG = G::TG, LPT = LPTG;
    constexpr int GSZ = (G::NU + LPTG - 1) / LPTG;  // threads of one loader group
    static_assert(NLG == 1 || (GSZ % 64 == 0 && NLG * GSZ <= G::THREADS), "loader groups");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, h = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hb = G::NH == 1 ? 0 : (blockIdx.x >> 3) & (G::NH - 1);
    const int chunk = G::NH == 1 ? blockIdx.x : ((blockIdx.x & 7) | ((blockIdx.x >> (3 + G::LNH)) << 3));
    if (chunk >= nchunk) return;
    const int64_t beg = (int64_t)chunk * rpc;
    const int64_t end = (beg + rpc < rows) ? beg + rpc : rows;
    // this wave's group pair (GA <= GB), row-major over the upper triangle of NTG x NTG
    int GA = 0, GB = 0;
    {
        int rem = hb * G::NWW + w;
        while (rem >= G::NTG - GA) {
            rem -= G::NTG - GA;
            ++GA;
        }
        GB = GA + rem;
    }
    f32x4 acc[TG][TG];
#pragma unroll
    for (int i = 0; i < TG; ++i)
#pragma unroll
        for (int j = 0; j < TG; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // thread unit u = tid + THREADS t (u < NU): rows kr = 4 (u & 7) .. + 3 of columns 4 (u >> 3) .. + 3
    float4 reg[LPT][4];
    // (the unit guard is wave-uniform -- NU is a multiple of 64 -- and a full step loads unguarded: a
    // per-load guard compiled to an exec branch per load; the partial last step clamps and zeroes)
    auto load = [&](int64_t r0) {
        const bool full = r0 + 32 <= end;
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            const int u = (NLG == 1 ? tid : tid % GSZ) + (NLG == 1 ? G::THREADS : GSZ) * t;
            if (u - lane >= G::NU) break;
            const int64_t row = r0 + 4 * (u & 7);
            const int c = 4 * (u >> 3);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (full) {
                    reg[t][q] = *reinterpret_cast<const float4*>(P + (row + q) * LP + c);
                } else {
                    const int64_t rr = row + q < end ? row + q : end - 1;
                    const float4 x = *reinterpret_cast<const float4*>(P + rr * LP + c);
                    reg[t][q] = row + q < end ? x : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
    };
    auto stage = [&](char* img) {
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            const int u = (NLG == 1 ? tid : tid % GSZ) + (NLG == 1 ? G::THREADS : GSZ) * t;
            if (u >= G::NU) break;
            const int kr = 4 * (u & 7);
            const int c0 = 4 * (u >> 3);
            const int rot = (u >> 3) & 3;  // octets write columns of alternating parity (LDS banks)
#pragma unroll
            for (int i0 = 0; i0 < 4; ++i0) {
                const int i = (i0 + rot) & 3;
                const int c = c0 + i;
                uint32_t pw[3][2];
#pragma unroll
                for (int q = 0; q < 4; q += 2) {
                    const float4 f0 = reg[t][q], f1 = reg[t][q + 1];
                    const float a = i == 0 ? f0.x : (i == 1 ? f0.y : (i == 2 ? f0.z : f0.w));
                    const float b = i == 0 ? f1.x : (i == 1 ? f1.y : (i == 2 ? f1.z : f1.w));
                    // exact three-piece split, two rows at a time: h = bf16(v), m = bf16(v - h), t = v - h - m
                    const uint32_t ph = cvt_pk_bf16(a, b);
                    const float ra = a - __uint_as_float(ph << 16), rb = b - __uint_as_float(ph & 0xffff0000u);
                    const uint32_t pm = cvt_pk_bf16(ra, rb);
                    const float ta = ra - __uint_as_float(pm << 16), tb = rb - __uint_as_float(pm & 0xffff0000u);
                    pw[0][q >> 1] = ph;
                    pw[1][q >> 1] = pm;
                    pw[2][q >> 1] = cvt_pk_bf16(ta, tb);
                }
                // rows kr .. kr + 3 of column c: 8 B inside 16-B unit kr >> 3 (swizzled), offset 8 ((kr >> 2) & 1)
                const int off = c * 64 + 16 * ((kr >> 3) ^ ((c >> 1) & 3)) + 8 * ((kr >> 2) & 1);
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    *reinterpret_cast<uint2*>(img + x * G::IMG + off) = make_uint2(pw[x][0], pw[x][1]);
            }
        }
    };
    const uint32_t lo = (uint32_t)(r * 64 + 16 * (h ^ ((r >> 1) & 3)));
    auto frag = [&](const char* img, int piece, int t) {
        return *reinterpret_cast<const bf16x8s*>(img + piece * G::IMG + t * 1024 + lo);
    };
    int buf = 0;
    // loader group of this wave (NLG > 1): it stages steps lg, lg + NLG, ... and loads NLG ahead
    const int lg = NLG == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid / GSZ);
    if (NLG == 1) {
        if (beg < end) load(beg);
    } else if (lg < NLG && beg + 32 * lg < end) {
        load(beg + 32 * lg);
    }
    int sm = 0;  // step index mod NLG
    for (int64_t r0 = beg; r0 < end; r0 += 32) {
        char* img = smem_raw + buf * G::STEP;
        if (G::NBUF == 1) __syncthreads();  // single buffer: the previous step's reads are done
        if (NLG == 1) {
            stage(img);
            __syncthreads();
            if (r0 + 32 < end) load(r0 + 32);
        } else {
            static_assert(NLG == 1 || G::NBUF == 2, "loader groups need two buffers");
            if (sm == lg) {
                stage(img);
                if (r0 + 32 * NLG < end) load(r0 + 32 * NLG);
            }
            sm = sm + 1 == NLG ? 0 : sm + 1;
            __syncthreads();
        }
        bf16x8s fa[TG][3];
#pragma unroll
        for (int i = 0; i < TG; ++i)
#pragma unroll
            for (int x = 0; x < 3; ++x) fa[i][x] = frag(img, x, GA * TG + i);
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            const bf16x8s hb_ = frag(img, 0, GB * TG + j), mb = frag(img, 1, GB * TG + j), tb = frag(img, 2, GB * TG + j);
#pragma unroll
            for (int i = 0; i < TG; ++i) {
                f32x4 c = acc[i][j];
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], hb_, c, 0, 0, 0);  // smallest terms first
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], tb, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], mb, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], hb_, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], mb, c, 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], hb_, c, 0, 0, 0);
            }
        }
        buf = G::NBUF - 1 - buf;
    }
#pragma unroll
    for (int i = 0; i < TG; ++i)
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            const int ta = GA * TG + i, tb = GB * TG + j;
            if (ta > tb) continue;  // (diagonal group pairs) the mirror of an upper pair
            const int a = ta >> 1, b = tb >> 1;
            const int blk = a * G::NB - a * (a - 1) / 2 + (b - a);
            double* dst = slabs + ((int64_t)chunk * G::NBLK + blk) * 1024;
            const bool mirror = (a == b) && (ta != tb);
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // bf16 MFMA D: col = lane & 15, row = 4 h + e
                const int li = 16 * (ta & 1) + 4 * h + e, lj = 16 * (tb & 1) + r;
                dst[li * 32 + lj] = (double)acc[i][j][e];
                if (mirror) dst[lj * 32 + li] = (double)acc[i][j][e];
            }
        }
}

// LP = 512, round 4: the same arithmetic (six bf16 products per tile pair, fp32 chunk accumulators,
// the same slabs) with each of a chunk's workgroups staging ONLY the column groups its group pairs
// read.  gram_split_kernel<512> staged all 512 columns (96 KB per 32-row step) in each of four
// workgroups: single-buffered, the VALU split work (430 instructions per wave per step) run 4x over
// between barriers, 168 VGPRs with spills at 9 waves -- rocprofv3: MFMA busy 23 %, waves parked
// 61 %, LDS 11 % busy.  Here the 36 group pairs of the 8 column groups (64 columns each) are dealt
// to five 8-wave workgroup types, each reading at most 6 groups:
//   0: groups {0,1,2,3}, pairs (0,0) (0,1) (0,2) (1,1) (1,2) (2,2) (0,3) (1,3)
//   1: groups {4,5,6,7}, the same pairs shifted by 4
//   2: {0,1} x {4,5,6,7}    3: {2,3} x {4,5,6,7}    4: (2,3) (3,3) (6,7) (7,7)
// so a step is at most 6 groups (72 KB): two buffers fit the LDS and the next step's split is
// staged while this step's MFMAs run (one barrier per step), at 2 waves per SIMD (256 VGPRs).
struct GramSplit4 {
    static constexpr int LP = 512, TG = 4, NB = 16, NBLK = NB * (NB + 1) / 2;
    static constexpr int TYPES = 5, WAVES = 12, THREADS = 64 * WAVES;  // 8 MFMA waves + 4 staging waves
    static constexpr int CWAVES = 8, SWAVES = WAVES - CWAVES;
    static constexpr int MAXG = 6;                 // staged groups (64 columns) per workgroup, at most
    static constexpr int IMG = MAXG * 64 * 64;     // bytes of one piece image (6 x 64 columns x 32 rows bf16)
    static constexpr int STEP = 3 * IMG;           // one 32-row step, three pieces (72 KB)
    static constexpr int LDS = 2 * STEP;           // double-buffered: 144 KB
    static constexpr int LPT = (MAXG * 64 * 4 + 64 * SWAVES - 1) / (64 * SWAVES);  // 8-row units per staging thread
};

// global group of local staged group lg, for workgroup type ty
__device__ __forceinline__ int gs4_group(int ty, int lg) {
    switch (ty) {
        case 0: return lg;
        case 1: return 4 + lg;
        case 2: return lg < 2 ? lg : 2 + lg;
        case 3: return 2 + lg;
        default: return lg < 2 ? 2 + lg : 4 + lg;
    }
}

__global__ __launch_bounds__(GramSplit4::THREADS) void gram_split4_kernel(const float* __restrict__ P, int64_t rows,
                                                                         int64_t rpc, int nchunk,
                                                                         double* __restrict__ slabs) {
    typedef GramSplit4 G;
    constexpr int TG = G::TG, LPT = G::LPT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, h = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    // a chunk's five workgroups are 8 apart in dispatch order: one XCD (its L2 serves the repeats)
    const int v = blockIdx.x >> 3;
    const int ty = v % G::TYPES;
    const int chunk = ((v / G::TYPES) << 3) | (blockIdx.x & 7);
    if (chunk >= nchunk) return;
    const int64_t beg = (int64_t)chunk * rpc;
    const int64_t end = (beg + rpc < rows) ? beg + rpc : rows;
    const int ngl = (ty == 2 || ty == 3) ? 6 : 4;  // staged groups
    const int NU = ngl * 64 * 4;                  // units of a step
    // this wave's group pair: local (LA <= LB) and global (GA <= GB)
    int LA, LB;
    bool active = true;
    if (ty < 2) {
        LA = (0x10211000 >> (4 * w)) & 15;  // w = 0..7: 0 0 0 1 1 2 0 1
        LB = (0x33221210 >> (4 * w)) & 15;  //          0 1 2 1 2 2 3 3
    } else if (ty < 4) {
        LA = w >> 2;
        LB = 2 + (w & 3);
    } else {
        LA = w & 3;
        LB = (w & 2) ? 3 : 1;
        active = w < 4;
    }
    const bool stager = w >= G::CWAVES;
    if (stager) active = false;
    const int sid = tid - 64 * G::CWAVES;  // staging thread index (stagers only)
    const int GA = gs4_group(ty, LA), GB = gs4_group(ty, LB);
    f32x4 acc[TG][TG];
#pragma unroll
    for (int i = 0; i < TG; ++i)
#pragma unroll
        for (int j = 0; j < TG; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (stager) {  // the staging waves: their own loop, the same barriers as the MFMA waves'
        // unit u = sid + 256 t (u < NU): row octet u / ncol (8 rows) of local column u % ncol.  A wave's
        // lanes take 64 consecutive columns (256-B row segments per load), each lane splits its 8 rows into
        // the three pieces with no component selects, and writes one 16-B octet per piece.  LDS image as
        // gram_split_kernel's: column c's 32 rows as four 16-B octets, octet o at o ^ ((c >> 1) & 3) -- 8
        // consecutive columns of a ds_write_b128 lane group hit 8 distinct slots, the fragment reads'
        // 16-lane groups 16.  Offsets are fixed for the launch: computed once.
        const int ncol = ngl * 64;
        int64_t goff[LPT];
        int loff[LPT];
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            const int u = sid + 64 * G::SWAVES * t;
            const int oc = u / ncol, lc = u - oc * ncol;
            goff[t] = (int64_t)(8 * oc) * G::LP + ((gs4_group(ty, lc >> 6) << 6) | (lc & 63));
            loff[t] = u < NU ? lc * 64 + 16 * (oc ^ ((lc >> 1) & 3)) : -1;
        }
        // two steps of loads in flight (a step's stage is ~1 us of work, an HBM round trip under this
        // load longer): register sets A and B alternate, loads issued two steps ahead of their stage
        typedef float Regs[LPT][8];
        Regs ra, rb;
        // (every guard is wave-uniform: no per-load exec branches -- they were 10 instructions per load;
        // the rows of a chunk's partial last step are clamped and zeroed)
        const int tmax = ngl == 6 ? LPT : 4;  // units t >= tmax do not exist for the 4-group types
        auto load = [&](Regs& reg, int64_t r0) {
            const bool full = r0 + 32 <= end;
#pragma unroll
            for (int t = 0; t < LPT; ++t) {
                if (t >= tmax) break;
                if (full) {
                    const float* src = P + r0 * G::LP + goff[t];
#pragma unroll
                    for (int q = 0; q < 8; ++q) reg[t][q] = src[q * G::LP];
                } else {
                    const int64_t row = r0 + (goff[t] >> 9);  // + 8 oc (G::LP = 512)
                    const int gc = (int)(goff[t] & (G::LP - 1));
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int64_t rr = row + q < end ? row + q : end - 1;
                        const float x = P[rr * G::LP + gc];
                        reg[t][q] = row + q < end ? x : 0.f;
                    }
                }
            }
        };
        auto stage = [&](const Regs& reg, char* img) {
#pragma unroll
            for (int t = 0; t < LPT; ++t) {
                if (t >= tmax) break;
                uint32_t pw[3][4];
#pragma unroll
                for (int q = 0; q < 8; q += 2) {
                    // exact three-piece split, two rows at a time: h = bf16(v), m = bf16(v - h), t = v - h - m
                    const float a = reg[t][q], b = reg[t][q + 1];
                    const uint32_t ph = cvt_pk_bf16(a, b);
                    const float ra_ = a - __uint_as_float(ph << 16), rb_ = b - __uint_as_float(ph & 0xffff0000u);
                    const uint32_t pm = cvt_pk_bf16(ra_, rb_);
                    const float ta = ra_ - __uint_as_float(pm << 16), tb = rb_ - __uint_as_float(pm & 0xffff0000u);
                    pw[0][q >> 1] = ph;
                    pw[1][q >> 1] = pm;
                    pw[2][q >> 1] = cvt_pk_bf16(ta, tb);
                }
#pragma unroll
                for (int x = 0; x < 3; ++x)
                    *reinterpret_cast<uint4*>(img + x * G::IMG + loff[t]) = make_uint4(pw[x][0], pw[x][1], pw[x][2], pw[x][3]);
            }
        };
        if (beg < end) {
            load(ra, beg);
            stage(ra, smem_raw);
            if (beg + 32 < end) load(rb, beg + 32);
            if (beg + 64 < end) load(ra, beg + 64);
        }
        __syncthreads();
        // iteration of step r0: stage step r0 + 32 into the other buffer (its last readers passed the
        // previous barrier) from the set loaded two iterations ago, then reload that set with r0 + 96
        auto iter = [&](Regs& reg, int64_t r0, int b) {
            if (r0 + 32 < end) {
                stage(reg, smem_raw + (b ^ 1) * G::STEP);
                if (r0 + 96 < end) load(reg, r0 + 96);
            }
            __syncthreads();
        };
        for (int64_t r0 = beg; r0 < end; r0 += 64) {
            iter(rb, r0, 0);
            if (r0 + 32 < end) iter(ra, r0 + 32, 1);
        }
        return;
    }
    const uint32_t lo = (uint32_t)(r * 64 + 16 * (h ^ ((r >> 1) & 3)));
    auto frag = [&](const char* img, int piece, int t) {  // t: local tile (16 columns)
        return *reinterpret_cast<const bf16x8s*>(img + piece * G::IMG + t * 1024 + lo);
    };
    __syncthreads();  // step 0 staged
    int buf = 0;
    for (int64_t r0 = beg; r0 < end; r0 += 32) {
        const char* img = smem_raw + buf * G::STEP;
        if (active) {
            bf16x8s fa[TG][3];
#pragma unroll
            for (int i = 0; i < TG; ++i)
#pragma unroll
                for (int x = 0; x < 3; ++x) fa[i][x] = frag(img, x, LA * TG + i);
#pragma unroll
            for (int j = 0; j < TG; ++j) {
                const bf16x8s hb_ = frag(img, 0, LB * TG + j), mb = frag(img, 1, LB * TG + j),
                              tb = frag(img, 2, LB * TG + j);
#pragma unroll
                for (int i = 0; i < TG; ++i) {
                    f32x4 c = acc[i][j];
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], hb_, c, 0, 0, 0);  // smallest terms first
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], tb, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], mb, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], hb_, c, 0, 0, 0);
                    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], mb, c, 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], hb_, c, 0, 0, 0);
                }
            }
        }
        __syncthreads();
        buf ^= 1;
    }
    if (!active) return;
#pragma unroll
    for (int i = 0; i < TG; ++i)
#pragma unroll
        for (int j = 0; j < TG; ++j) {
            const int ta = GA * TG + i, tb = GB * TG + j;
            if (ta > tb) continue;  // (diagonal group pairs) the mirror of an upper pair
            const int a = ta >> 1, b = tb >> 1;
            const int blk = a * G::NB - a * (a - 1) / 2 + (b - a);
            double* dst = slabs + ((int64_t)chunk * G::NBLK + blk) * 1024;
            const bool mirror = (a == b) && (ta != tb);
#pragma unroll
            for (int e = 0; e < 4; ++e) {  // bf16 MFMA D: col = lane & 15, row = 4 h + e
                const int li = 16 * (ta & 1) + 4 * h + e, lj = 16 * (tb & 1) + r;
                dst[li * 32 + lj] = (double)acc[i][j][e];
                if (mirror) dst[lj * 32 + li] = (double)acc[i][j][e];
            }
        }
}

}  // namespace

bool gram_split_ok(int LP) { return LP == 128 || LP == 256 || LP == 512; }

hipError_t launch_gram_split(const float* P, int64_t rows, int LP, const GramPlan& gp, double* slabs, double* G,
                             hipStream_t s) {
    if (!gram_split_ok(LP)) return hipErrorInvalidValue;
    int nchunk = gp.chunks;
    auto go = [&](auto lpc) {
        constexpr int L = decltype(lpc)::value;
        if constexpr (L == 512) {  // gram_split4_kernel on chunks of its own
            // one round of 5-workgroup chunks on the 256 CUs (51 x 5 = 255), >= 512 rows each, within the
            // plan's slab count (the fp32 accumulators then run over up to ~2600 rows, as C3's 4096 do)
            int64_t ch = (rows + 511) / 512;
            if (ch > 51) ch = 51;
            if (ch > gp.chunks) ch = gp.chunks;
            if (ch < 1) ch = 1;
            int64_t rpc = (rows + ch - 1) / ch;
            rpc = rpc < 32 ? 32 : (rpc + 31) / 32 * 32;  // (a rank's shard may hold no rows: one empty chunk)
            nchunk = rows > 0 ? (int)((rows + rpc - 1) / rpc) : 1;
            hipLaunchKernelGGL(gram_split4_kernel, dim3((nchunk + 7) / 8 * 8 * GramSplit4::TYPES),
                               dim3(GramSplit4::THREADS), GramSplit4::LDS, s, P, rows, rpc, nchunk, slabs);
        } else {
            typedef GramSplit<L> GS;
            const int grid = GS::NH == 1 ? gp.chunks : (gp.chunks + 7) / 8 * 8 * GS::NH;
            if constexpr (L == 128) {  // two loader groups taking the steps in turn (round 4, 220 -> 180 us at C3)
                hipLaunchKernelGGL((gram_split_kernel<L, 1, 2>), dim3(grid), dim3(GS::THREADS), GS::NBUF * GS::STEP, s,
                                   P, rows, gp.rows_per_chunk, gp.chunks, slabs);
                return;
            }
            hipLaunchKernelGGL(gram_split_kernel<L>, dim3(grid), dim3(GS::THREADS), GS::NBUF * GS::STEP, s, P, rows,
                               gp.rows_per_chunk, gp.chunks, slabs);
        }
    };
    if (LP == 128) go(std::integral_constant<int, 128>{});
    else if (LP == 256) go(std::integral_constant<int, 256>{});
    else go(std::integral_constant<int, 512>{});
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_gram_reduce(slabs, gp.blocks, nchunk, LP, 0, G, nullptr, s);
}

namespace {

// Cross Gram R = X^T Y of two fp32 panels at LP = 256 / 512 by the same three-piece bf16 split (round
// 4: R = Q_B^T B^T, the fp64-MFMA gram_wide_kernel<float, true> took 237 us at C4 for 8.6 GFLOP).
// Workgroup types per row chunk: the 64 columns of X's group gx against 256 columns (half gy) of Y
// -- 4 types at LP = 256, 16 at LP = 512.  A step stages 64 + 256 columns (octet units as
// gram_split4_kernel, 60 KB, double-buffered); wave w takes X tiles 2 (w & 1) .. + 1 of the group and
// Y tiles 4 (w >> 1) .. + 3 of the half -- 8 tile pairs, six MFMAs each.  Partial 32 x 32 blocks go
// to the cross slab layout gram_reduce4_kernel sums (blk = a nb + b).
template <int LP_> struct GramSplitX {
    static constexpr int LP = LP_, NB = LP / 32, NBLK = NB * NB, WAVES = 8, THREADS = 64 * WAVES;
    static constexpr int GXN = LP / 64, GYN = LP / 256, TYPES = GXN * GYN;
    static constexpr int XC = 64, YC = 256;               // staged columns of X (one group) and Y (one half)
    static constexpr int XIMG = XC * 64, YIMG = YC * 64;  // bytes per piece image (32 rows bf16 per column)
    static constexpr int STEP = 3 * (XIMG + YIMG);        // 60 KB
    static constexpr int NU = 4 * (XC + YC);              // 8-row x 1-column units per step
    static constexpr int LPT = (NU + THREADS - 1) / THREADS;
};

template <int LP_>
__global__ __launch_bounds__(GramSplitX<LP_>::THREADS) void gram_split_cross_kernel(const float* __restrict__ X,
                                                                                   const float* __restrict__ Y,
                                                                                   int64_t rows, int64_t rpc,
                                                                                   int nchunk,
                                                                                   double* __restrict__ slabs) {
    typedef GramSplitX<LP_> G;
    constexpr int LPT = G::LPT;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 15, h = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int v = blockIdx.x >> 3;  // a chunk's types are 8 apart in dispatch order: one XCD
    const int ty = v % G::TYPES;
    const int gx = ty % G::GXN, gy = ty / G::GXN;
    const int chunk = ((v / G::TYPES) << 3) | (blockIdx.x & 7);
    if (chunk >= nchunk) return;
    const int64_t beg = (int64_t)chunk * rpc;
    const int64_t end = (beg + rpc < rows) ? beg + rpc : rows;
    const int xt0 = 2 * (w & 1), yt0 = 4 * (w >> 1);  // local X tiles (of the group), Y tiles
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // unit u: units [0, 4 XC) are X's (octet u / XC of local column u % XC), the rest Y's
    int oct[LPT], coff[LPT], loff[LPT];
    bool isx[LPT];
#pragma unroll
    for (int t = 0; t < LPT; ++t) {
        const int u = tid + G::THREADS * t;
        const bool xu = u < 4 * G::XC;
        const int uu = xu ? u : u - 4 * G::XC;
        const int nc = xu ? G::XC : G::YC;
        const int oc = uu / nc, c = uu - oc * nc;
        isx[t] = xu;
        oct[t] = 8 * oc;
        coff[t] = xu ? 64 * gx + c : 256 * gy + c;
        loff[t] = (u < G::NU) ? (xu ? 0 : 3 * G::XIMG) + c * 64 + 16 * (oc ^ ((c >> 1) & 3)) : -1;
    }
    float reg[LPT][8];
    auto load = [&](int64_t r0) {
        const bool full = r0 + 32 <= end;
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            if (tid + G::THREADS * t - lane >= G::NU) break;  // wave-uniform (NU, THREADS multiples of 64)
            const float* base = isx[t] ? X : Y;
            const int64_t row = r0 + oct[t];
            if (full) {
                const float* src = base + row * G::LP + coff[t];
#pragma unroll
                for (int q = 0; q < 8; ++q) reg[t][q] = src[q * G::LP];
            } else {  // the chunk's partial last step: rows clamped and zeroed
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int64_t rr = row + q < end ? row + q : end - 1;
                    const float x = base[rr * G::LP + coff[t]];
                    reg[t][q] = row + q < end ? x : 0.f;
                }
            }
        }
    };
    auto stage = [&](char* img) {
#pragma unroll
        for (int t = 0; t < LPT; ++t) {
            if (loff[t] < 0) break;
            uint32_t pw[3][4];
#pragma unroll
            for (int q = 0; q < 8; q += 2) {
                const float a = reg[t][q], b = reg[t][q + 1];
                const uint32_t ph = cvt_pk_bf16(a, b);
                const float ra = a - __uint_as_float(ph << 16), rb = b - __uint_as_float(ph & 0xffff0000u);
                const uint32_t pm = cvt_pk_bf16(ra, rb);
                const float ta = ra - __uint_as_float(pm << 16), tb = rb - __uint_as_float(pm & 0xffff0000u);
                pw[0][q >> 1] = ph;
                pw[1][q >> 1] = pm;
                pw[2][q >> 1] = cvt_pk_bf16(ta, tb);
            }
            const int pstride = isx[t] ? G::XIMG : G::YIMG;
#pragma unroll
            for (int x = 0; x < 3; ++x)
                *reinterpret_cast<uint4*>(img + loff[t] + x * pstride) = make_uint4(pw[x][0], pw[x][1], pw[x][2], pw[x][3]);
        }
    };
    const uint32_t lo = (uint32_t)(r * 64 + 16 * (h ^ ((r >> 1) & 3)));
    if (beg < end) {
        load(beg);
        stage(smem_raw);
        if (beg + 32 < end) load(beg + 32);
    }
    __syncthreads();
    int buf = 0;
    for (int64_t r0 = beg; r0 < end; r0 += 32) {
        const char* img = smem_raw + buf * G::STEP;
        bf16x8s fa[2][3];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int x = 0; x < 3; ++x)
                fa[i][x] = *reinterpret_cast<const bf16x8s*>(img + x * G::XIMG + (xt0 + i) * 1024 + lo);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const char* yb = img + 3 * G::XIMG + (yt0 + j) * 1024 + lo;
            const bf16x8s yh = *reinterpret_cast<const bf16x8s*>(yb), ym = *reinterpret_cast<const bf16x8s*>(yb + G::YIMG),
                          yt = *reinterpret_cast<const bf16x8s*>(yb + 2 * G::YIMG);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                f32x4 c = acc[i][j];
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][2], yh, c, 0, 0, 0);  // smallest terms first
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], yt, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], ym, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][1], yh, c, 0, 0, 0);
                c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], ym, c, 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i][0], yh, c, 0, 0, 0);
            }
        }
        if (r0 + 32 < end) {
            stage(smem_raw + (buf ^ 1) * G::STEP);
            if (r0 + 64 < end) load(r0 + 64);
        }
        __syncthreads();
        buf ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ta = 4 * gx + xt0 + i, tb = 16 * gy + yt0 + j;  // global 16-column tiles of X, Y
            const int blk = (ta >> 1) * G::NB + (tb >> 1);
            double* dst = slabs + ((int64_t)chunk * G::NBLK + blk) * 1024;
#pragma unroll
            for (int e = 0; e < 4; ++e)  // bf16 MFMA D: col = lane & 15, row = 4 h + e
                dst[(16 * (ta & 1) + 4 * h + e) * 32 + 16 * (tb & 1) + r] = (double)acc[i][j][e];
        }
}

}  // namespace

hipError_t launch_gram_split_cross(const float* X, const float* Y, int64_t rows, int LP, const GramPlan& gp,
                                   double* slabs, double* G, hipStream_t s) {
    if ((LP != 256 && LP != 512) || gp.blocks != (LP / 32) * (LP / 32)) return hipErrorInvalidValue;
    // >= 256 rows per chunk, at most the plan's chunk count (its slabs), ~256 workgroups
    const int types = LP == 256 ? GramSplitX<256>::TYPES : GramSplitX<512>::TYPES;
    int64_t ch = (rows + 255) / 256;
    if (ch > 256 / types) ch = 256 / types;
    if (ch > gp.chunks) ch = gp.chunks;
    if (ch < 1) ch = 1;
    int64_t rpc = (rows + ch - 1) / ch;
    rpc = (rpc + 31) / 32 * 32;
    // each fp32 MFMA accumulator sums one chunk's rows; past kSplitCrossRows per chunk (n > 262144 at
    // LP = 256, n > 65536 at LP = 512) its error would grow with n -- the fp64 cross Gram instead
    if (rpc > kSplitCrossRows) return launch_gram_wide<float>(X, Y, rows, LP, gp, slabs, G, nullptr, s);
    const int nchunk = (int)((rows + rpc - 1) / rpc);
    const dim3 grid((unsigned)((nchunk + 7) / 8 * 8 * types));
    if (LP == 256)
        hipLaunchKernelGGL(gram_split_cross_kernel<256>, grid, dim3(GramSplitX<256>::THREADS), 2 * GramSplitX<256>::STEP,
                           s, X, Y, rows, rpc, nchunk, slabs);
    else
        hipLaunchKernelGGL(gram_split_cross_kernel<512>, grid, dim3(GramSplitX<512>::THREADS), 2 * GramSplitX<512>::STEP,
                           s, X, Y, rows, rpc, nchunk, slabs);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_gram_reduce(slabs, gp.blocks, nchunk, LP, 1, G, nullptr, s);
}

}  // namespace rsvd
