// wide_chol.hip -- R = chol(G) and R^-1 of the wide engine's CholeskyQR (wide.hpp): the 16x16 diagonal
// factors, the one-workgroup kernels (chol_wide, chol_reg, rinv_wide), the two-level factor on the fp64
// MFMA GEMM, and launch_chol, which chooses between them.
#include <algorithm>
#include <type_traits>

#include "wide_dev.hpp"

namespace rsvd {

namespace {

// ------------------------------------------------------------------------------------------------
// Cholesky, one workgroup of kCholThreads threads.  W (work) holds the Gram being reduced (upper
// block triangle only); R gets the factor's upper block triangle, Rinv the inverse diagonal blocks
// (rinv_wide_kernel fills the rest).  Per 16-column block p: the strip R[p][p+1..] = D_p^-T W[p][p+1..]
// (to global R and an LDS copy), then the trailing update W -= R[p]^T R[p] on the fp64 MFMA with both
// operands from the LDS strip, each wave keeping kCholBatch W tiles' read-modify-write in flight (one
// CU's update is latency-bound otherwise).  Look-ahead: wave 0 updates tile (p+1, p+1) first and
// factors it -- 16x16 upper Cholesky and inverse in registers, lane j owning column j, pivots and rows
// broadcast on the 64-bit DPP, rsqrt + Newton pivots -- while the other waves finish the update.  Two
// workgroup barriers per block.
constexpr int kCholThreads = 512;
constexpr int kCholBatch = 6;
constexpr int kCholPad = 16;  // LDS strip pitch LP + 16 doubles: the 4 k-rows of a tile read hit different banks

__device__ __forceinline__ void tri_decode(int t, int nt2, int& ib, int& jb) {  // t -> (ib <= jb) in [0, nt2)
    int rem = t, i = 0;
    while (rem >= nt2 - i) {
        rem -= nt2 - i;
        ++i;
    }
    ib = i;
    jb = i + rem;
}

// 1/sqrt(d) to fp64 accuracy: hardware estimate + two Newton steps
__device__ __forceinline__ double rsqrt_nr(double d) {
    double y = __builtin_amdgcn_rsq(d);
    y = y * fma(-0.5 * d * y, y, 1.5);
    y = y * fma(-0.5 * d * y, y, 1.5);
    return y;
}

// Wave-level factor of a 16x16 diagonal block for the single-wave critical path of the block
// Cholesky (lane j: col[i] = T[i][j]; the upper part is valid).  Measured: the predicated form
// (`if (j >= i) col[i] -= ...`) followed by a separate back substitution ran 6 us per block, a
// dependent chain of ~2000 VALU/readlane instructions on one wave.  Here every update is
// unconditional (lanes j < i only carry lower-triangle values no later step reads), and D^-1 is
// formed in the same pivot loop: row k of Y = D^-T (lane j: Y[k][j] = D^-1[j][k]) is
// (e_j[k] - acc[k]) / D[k][k], and each broadcast D[k][i] feeds both the factor update and
// acc[i] += D[k][i] Y[k][j].  Writes the R and R^-1 diagonal blocks (global), D^-1 (Di, LDS,
// row-major), the breakdown rows (bad) and flags.
// The row broadcasts run on the 64-bit DPP of gfx90a+ (row_newbcast:i -- lane i of every 16-lane row
// to the whole row): the tile is replicated in the wave's four rows (lane j of each row owns column
// j), so D[k][i] = lane i's col[k] reaches every lane of the row inside the FMA that uses it --
// v_fmac_f64_dpp, ONE instruction per update instead of two v_readlane (SGPRs, which the compiler
// hoisted and spilled) and an FMA.  The d0 diagonal of the block is read before the pivot chain
// (lane j: d0[p16 + j], broadcast per pivot).  The asm carries `s_nop 1` for the VALU-write ->
// DPP-read hazard (the compiler's hazard recognizer does not look into inline asm).
template <int I>
__device__ __forceinline__ double nbcast_f64(double v) {
    double r;
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(v), "i"(I));
    return r;
}
template <int I>
__device__ __forceinline__ void fmac_nbcast_f64(double& acc, double x, double y) {  // acc += x[lane I of the row] * y
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
        : "+v"(acc)
        : "v"(x), "v"(y), "i"(I));
}
template <int K, int I>
__device__ __forceinline__ void diag16_updates(double (&col)[16], double (&acc)[16], double ck, double nck, double yk) {
    if constexpr (I < 16) {
        fmac_nbcast_f64<I>(col[I], ck, nck);  // col[i] -= D[k][i] col[k]
        fmac_nbcast_f64<I>(acc[I], ck, yk);   // acc[i] += D[k][i] Y[k][j]
        diag16_updates<K, I + 1>(col, acc, ck, nck, yk);
    }
}
template <int K>
__device__ __forceinline__ void diag16_pivots(double (&col)[16], double (&acc)[16], int j, int p16, int l, double tol,
                                              double d0j, double* Di, int lane, int& badmask) {
    if constexpr (K < 16) {
        const int gk = p16 + K;
        const double dkk = nbcast_f64<K>(col[K]);
        const double d0k = nbcast_f64<K>(d0j);
        const bool pad = gk >= l;
        const bool isbad = !pad && (!(dkk > tol * d0k) || !(d0k > 0.0) || !isfinite(dkk));
        if (isbad) badmask |= 1 << K;
        const bool unit = pad || isbad;
        const double y = unit ? 1.0 : rsqrt_nr(dkk);
        const double rk = unit ? 1.0 : dkk * y;
        const double v = unit ? 0.0 : col[K] * y;
        col[K] = (j == K) ? rk : v;
        const double yk = ((j == K ? 1.0 : 0.0) - acc[K]) * y;  // Y[k][j] = D^-1[j][k]
        if (lane < 16) Di[j * 16 + K] = yk;
        diag16_updates<K, K + 1>(col, acc, col[K], -col[K], yk);
        diag16_pivots<K + 1>(col, acc, j, p16, l, tol, d0j, Di, lane, badmask);
    }
}
__device__ __forceinline__ void chol_diag16_dpp(double (&col)[16], int p16, int l, int LP, double tol, const double* d0,
                                                double* Di, int* bad, double* R, double* Rinv, int* colflag, int* flag,
                                                int lane) {
    const int j = lane & 15;
    const double d0j = d0[p16 + j];
    int badmask = 0;  // the same in every lane (uniform tests)
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0;
    diag16_pivots<0>(col, acc, j, p16, l, tol, d0j, Di, lane, badmask);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i > j) col[i] = 0.0;
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) R[(int64_t)(p16 + i) * LP + p16 + j] = col[i];
        bad[lane] = (badmask >> lane) & 1;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's D^-1 rows landed
    __builtin_amdgcn_wave_barrier();
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; i += 2)
            *reinterpret_cast<double2*>(Rinv + (int64_t)(p16 + j) * LP + p16 + i) =
                *reinterpret_cast<const double2*>(Di + j * 16 + i);
    }
    if (lane == 0 && badmask) {
        atomicAdd(flag, __popc(badmask));
        for (int k = 0; k < 16; ++k)
            if (badmask & (1 << k)) colflag[p16 + k] = 1;
    }
}
// Round 5: the same factor with fewer instructions on the pivot loop.  One wave issues at most one
// instruction per four cycles, and the DPP form above spent 1686 instructions per factor (974 VALU,
// 712 SALU: s_nop hazards, exec-mask branches around the rsqrt and the D^-1 stores, per-pivot
// breakdown tests) -- 7844 cycles.  Here:
//  * the breakdown / finiteness tests leave the pivot loop: lane k keeps its pivot d_kk, and after
//    the loop one vector test (lane j judges pivot j) and a ballot decide; a bad or padding pivot
//    (rare: rank deficiency, l % 16) re-runs chol_diag16_dpp from the staged tile -- the only path
//    that needs the unit-pivot substitutions;
//  * rsqrt unconditional (no branch), the D^-1 rows stay in registers (lane j: row j of D^-1) and
//    are stored once after the loop (LDS Di and the global R^-1 block), no per-pivot exec masks;
//  * -col[K] is the DPP FMA's src1 negation modifier, and only the first DPP use of each pivot
//    row carries the `s_nop 1` (its source was just written); the later ones read it again.
// Same operations in the same order as chol_diag16_dpp on a pivot chain without breakdowns:
// bit-identical R and R^-1 (tools/wide_lab chol checks it).
template <int I>
__device__ __forceinline__ void fmsub_nbcast_nop(double& acc, double x, double y) {  // acc -= x[lane I] * y, hazard-safe
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(x), "v"(y), "i"(I));
}
// (volatile: kept in program order, so every hazard-free use follows the s_nop'ed first use)
template <int I>
__device__ __forceinline__ void fmsub_nbcast(double& acc, double x, double y) {  // x written >= 2 instrs earlier
    asm volatile("v_fmac_f64_dpp %0, %1, -%2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(x), "v"(y), "i"(I));
}
template <int I>
__device__ __forceinline__ void fmadd_nbcast(double& acc, double x, double y) {
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(x), "v"(y), "i"(I));
}
template <int K, int I>
__device__ __forceinline__ void diag16v2_updates(double (&col)[16], double (&acc)[16], double ck, double yk) {
    if constexpr (I < 16) {
        if constexpr (I == K + 1) fmsub_nbcast_nop<I>(col[I], ck, ck);  // col[i] -= D[k][i] col[k]
        else fmsub_nbcast<I>(col[I], ck, ck);
        fmadd_nbcast<I>(acc[I], ck, yk);  // acc[i] += D[k][i] Y[k][j]
        diag16v2_updates<K, I + 1>(col, acc, ck, yk);
    }
}
// `careful` (uniform): the breakdown / padding tests of chol_diag16_dpp on every pivot; a unit pivot
// (padding row or breakdown) is the same arithmetic on the substituted row e_k with d_kk = 1 (then
// y = rk = 1, v = 0, exactly the unit-pivot values of the DPP form).
template <int K>
__device__ __forceinline__ void diag16v2_pivots(double (&col)[16], double (&acc)[16], double (&yrow)[16], int j,
                                                double& dsave, bool careful, int p16, int l, double tol, double d0j,
                                                int& badmask) {
    if constexpr (K < 16) {
        double dkk = nbcast_f64<K>(col[K]);
        if (careful) {
            const double d0k = nbcast_f64<K>(d0j);
            const bool pad = p16 + K >= l;
            const bool isbad = !pad && (!(dkk > tol * d0k) || !(d0k > 0.0) || !isfinite(dkk));
            if (isbad) badmask |= 1 << K;
            if (pad || isbad) {
                dkk = 1.0;
                col[K] = (j == K) ? 1.0 : 0.0;
            }
        }
        dsave = (j == K) ? dkk : dsave;
        const double y = rsqrt_nr(dkk);
        const double rk = dkk * y;
        const double v = col[K] * y;
        col[K] = (j == K) ? rk : v;
        const double yk = ((j == K ? 1.0 : 0.0) - acc[K]) * y;  // Y[k][j] = D^-1[j][k]
        yrow[K] = yk;
        diag16v2_updates<K, K + 1>(col, acc, col[K], yk);
        diag16v2_pivots<K + 1>(col, acc, yrow, j, dsave, careful, p16, l, tol, d0j, badmask);
    }
}
// src: the staged tile (LDS, [i][16] row-major: src[i * 16 + j] = T[i][j]).  Pass 0 runs without the
// per-pivot tests; if a pivot then fails them (ballot) -- or the block has padding rows -- the same
// unrolled body runs again from src with the tests on (pass 1).
__device__ __forceinline__ void chol_diag16_v2(double (&col)[16], int p16, int l, int LP, double tol, const double* d0,
                                               double* Di, int* bad, double* R, double* Rinv, int* colflag, int* flag,
                                               int lane, const double* src) {
    const int j = lane & 15;
    const double d0j = d0[p16 + j];
    double acc[16], yrow[16];
    int badmask = 0;
    for (int pass = p16 + 16 > l ? 1 : 0;; ++pass) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.0;
        double dsave = 0.0;
        diag16v2_pivots<0>(col, acc, yrow, j, dsave, pass != 0, p16, l, tol, d0j, badmask);
        if (pass) break;
        // lane j judges its own pivot (the test chol_diag16_dpp applies per pivot)
        const bool isbad = !(dsave > tol * d0j) || !(d0j > 0.0) || !isfinite(dsave);
        if (!__ballot(isbad && lane < 16)) break;
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i] = src[i * 16 + j];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i > j) col[i] = 0.0;
    if (lane < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) R[(int64_t)(p16 + i) * LP + p16 + j] = col[i];
#pragma unroll
        for (int k = 0; k < 16; k += 2) {
            const double2 v2 = make_double2(yrow[k], yrow[k + 1]);
            *reinterpret_cast<double2*>(Di + j * 16 + k) = v2;
            *reinterpret_cast<double2*>(Rinv + (int64_t)(p16 + j) * LP + p16 + k) = v2;
        }
        bad[lane] = (badmask >> lane) & 1;
    }
    if (lane == 0 && badmask) {
        atomicAdd(flag, __popc(badmask));
        for (int k = 0; k < 16; ++k)
            if (badmask & (1 << k)) colflag[p16 + k] = 1;
    }
}

// The split-Gram fallback test after a factor (off the pivot chain): ill = some valid pivot broke
// down or R_kk^2 <= ill_tol G_kk.  Called by the whole workgroup after its last barrier (the R
// diagonal and colflag stores of the factor are then visible workgroup-wide).
__device__ __forceinline__ void chol_ill_test(const double* __restrict__ R, int LP, int l, const double* d0,
                                              const int* __restrict__ colflag, double ill_tol, int* ill,
                                              int* ill_s, int tid, int nthr) {
    int mine = 0;
    for (int k = tid; k < l; k += nthr) {
        const double rkk = R[(int64_t)k * LP + k];
        if (colflag[k] || !(rkk * rkk > ill_tol * d0[k])) mine = 1;
    }
    if (mine) *ill_s = 1;
    __syncthreads();
    if (tid == 0) *ill = *ill_s;
}

#ifdef RSVD_CHOL_PROF
__device__ long long g_chol_prof[256];
#define CHOL_TS(k)                                               \
    do {                                                         \
        if (threadIdx.x == 0) g_chol_prof[(k)] = wall_clock64(); \
    } while (0)
#else
#define CHOL_TS(k) \
    do {           \
    } while (0)
#endif

// Upper block-triangle walk (ib <= jb < n): advance by `step` tiles; ib >= n marks the end.
struct TriWalk {
    int ib, jb, n;
    __device__ __forceinline__ TriWalk(int t, int n_) : ib(n_), jb(0), n(n_) {
        if (t < n_ * (n_ + 1) / 2) tri_decode(t, n_, ib, jb);
    }
    __device__ __forceinline__ void advance(int step) {
        jb += step;
        while (ib < n && jb >= n) {
            const int over = jb - n;
            ++ib;
            jb = ib + over;
        }
    }
};

// W is kept tile-major in MFMA output order: tile (ib, jb) at (ib * np + jb) * 256, lane (r, h)'s
// four values (rows h + 4 j, column r) contiguous -- one 32-B access per lane per tile, and the
// same registers serve as the B operand (rows 4 kk + h) of the strip product.
__device__ __forceinline__ double* wtile(double* W, int np, int ib, int jb, int lane) {
    return W + ((int64_t)ib * np + jb) * 256 + lane * 4;
}

template <int NT, int B>
__global__ __launch_bounds__(NT) void chol_wide_kernel(const double* __restrict__ G, int l, int LP,
                                                                 double tol, double* __restrict__ W,
                                                                 double* __restrict__ R, double* __restrict__ Rinv,
                                                                 int* __restrict__ colflag, int* __restrict__ flag,
                                                                 const int* __restrict__ pred, double ill_tol,
                                                                 int* __restrict__ ill, const double* __restrict__ d0src,
                                                                 int ldg) {
    if (pred && *pred == 0) return;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ int ill_s;
    const int np = LP / 16;
    const int ldr = LP + kCholPad;
    constexpr int nw = NT / 64;
    double* Dd = reinterpret_cast<double*>(smem_raw);  // [2][16][16] D^-1 of blocks p, p+1
    double* d0 = Dd + 512;                             // [LP] original diagonal of G
    double* Rs = d0 + LP;                              // [16][ldr] current R row strip
    double* Tsc = Rs + 16 * ldr;                       // [16][16] wave 0's look-ahead tile
    int* bad = reinterpret_cast<int*>(Tsc + 256);      // [2][16]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, h = lane >> 4;
    CHOL_TS(97);

    // W := upper block triangle of G (zero beyond l), tile-major; B tiles per wave in flight
    {
        TriWalk tw(wv, np);
        while (tw.ib < np) {
            double v[B][4];
            int tix[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {
                tix[b] = tw.ib < np ? tw.ib * 64 + tw.jb : -1;
                if (tw.ib < np) {
                    const int c = 16 * tw.jb + r;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = 16 * tw.ib + h + 4 * j;
                        v[b][j] = (i < l && c < l) ? G[(int64_t)i * ldg + c] : 0.0;
                    }
                }
                tw.advance(nw);
            }
#pragma unroll
            for (int b = 0; b < B; ++b)
                if (tix[b] >= 0) {
                    double* dst = wtile(W, np, tix[b] >> 6, tix[b] & 63, lane);
                    *reinterpret_cast<double2*>(dst) = make_double2(v[b][0], v[b][1]);
                    *reinterpret_cast<double2*>(dst + 2) = make_double2(v[b][2], v[b][3]);
                }
        }
    }
    for (int i = tid; i < LP; i += NT) {
        d0[i] = (i < l) ? (d0src ? d0src[i] : G[(int64_t)i * ldg + i]) : 0.0;
        colflag[i] = 0;
    }
    if (tid == 0) ill_s = 0;
    __syncthreads();
    CHOL_TS(0);

    for (int p = -1; p < np; ++p) {  // p = -1: only the factor of diagonal block 0
        const int p16 = 16 * p;
        const double* Di = Dd + (p & 1) * 256;
        const int* bd = bad + (p & 1) * 16;
        // (1) strip R[p][jb] = D_p^-T W[p][jb] (0 for rows that broke down), to R and the LDS strip
        if (p >= 0) {
            double x[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) x[kk] = Di[(4 * kk + h) * 16 + r];
            int zero_rows = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) zero_rows |= (bd[h + 4 * j] || p16 + h + 4 * j >= l) << j;
            for (int jb0 = p + 1 + wv; jb0 < np; jb0 += nw * 4) {
                double2 y[4][2];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int jb = jb0 + nw * b;
                    if (jb < np) {
                        const double* src = wtile(W, np, p, jb, lane);
                        y[b][0] = *reinterpret_cast<const double2*>(src);
                        y[b][1] = *reinterpret_cast<const double2*>(src + 2);
                    }
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int jb = jb0 + nw * b;
                    if (jb < np) {
                        f64x4 acc = MD::zero();
                        acc = MD::mma(x[0], y[b][0].x, acc);
                        acc = MD::mma(x[1], y[b][0].y, acc);
                        acc = MD::mma(x[2], y[b][1].x, acc);
                        acc = MD::mma(x[3], y[b][1].y, acc);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int i = h + 4 * j;
                            const double v = ((zero_rows >> j) & 1) ? 0.0 : acc[j];
                            R[(int64_t)(p16 + i) * LP + 16 * jb + r] = v;
                            Rs[i * ldr + 16 * jb + r] = v;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (p >= 0) CHOL_TS(1 + 2 * p);
        // (2) trailing update W[ib][jb] -= R[p][ib]^T R[p][jb], p < ib <= jb.  Tile (p+1, p+1) goes to
        // wave 0, which then factors it (look-ahead); the other tiles to waves 1.., software-pipelined
        // in batches of B (loads of batch i+1 in flight while batch i is updated and stored).
        const int nt2 = np - p - 1;
        if (nt2 > 0) {
            if (wv == 0) {
                const int b1 = p + 1;
                const double* src = wtile(W, np, b1, b1, lane);
                const double2 w0 = *reinterpret_cast<const double2*>(src);
                const double2 w1 = *reinterpret_cast<const double2*>(src + 2);
                f64x4 acc = MD::zero();
                if (p >= 0) {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk)
                        acc = MD::mma(Rs[(4 * kk + h) * ldr + 16 * b1 + r], Rs[(4 * kk + h) * ldr + 16 * b1 + r], acc);
                }
                Tsc[h * 16 + r] = w0.x - acc[0];
                Tsc[(h + 4) * 16 + r] = w0.y - acc[1];
                Tsc[(h + 8) * 16 + r] = w1.x - acc[2];
                Tsc[(h + 12) * 16 + r] = w1.y - acc[3];
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave's LDS stores landed
                __builtin_amdgcn_wave_barrier();
                double col[16];
#pragma unroll
                for (int i = 0; i < 16; ++i) col[i] = Tsc[i * 16 + r];
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                // (the DPP form here: this factor overlaps the other waves' trailing updates, and the v2
                // form's extra registers spilled in this kernel -- LP = 512 637 -> 809 us in the lab)
                chol_diag16_dpp(col, 16 * b1, l, LP, tol, d0, Dd + (b1 & 1) * 256, bad + (b1 & 1) * 16, R, Rinv,
                                colflag, flag, lane);
            } else if (p >= 0) {
                // local tile t of the (nt2 x nt2) upper triangle; t = 0 is wave 0's
                TriWalk tw(wv, nt2);
                double2 wa[B][2], wb[B][2];
                int ta[B], tb[B];
                auto load = [&](double2 (&w)[B][2], int (&tt)[B]) {
#pragma unroll
                    for (int b = 0; b < B; ++b) {
                        tt[b] = tw.ib < nt2 ? tw.ib * 64 + tw.jb : -1;
                        if (tw.ib < nt2) {
                            const double* src = wtile(W, np, p + 1 + tw.ib, p + 1 + tw.jb, lane);
                            w[b][0] = *reinterpret_cast<const double2*>(src);
                            w[b][1] = *reinterpret_cast<const double2*>(src + 2);
                        }
                        tw.advance(nw - 1);
                    }
                };
                auto update = [&](double2 (&w)[B][2], int (&tt)[B]) {
#pragma unroll
                    for (int b = 0; b < B; ++b)
                        if (tt[b] >= 0) {
                            const int ib = p + 1 + (tt[b] >> 6), jb = p + 1 + (tt[b] & 63);
                            f64x4 acc = MD::zero();
#pragma unroll
                            for (int kk = 0; kk < 4; ++kk)
                                acc = MD::mma(Rs[(4 * kk + h) * ldr + 16 * ib + r], Rs[(4 * kk + h) * ldr + 16 * jb + r],
                                              acc);
                            double* dst = wtile(W, np, ib, jb, lane);
                            *reinterpret_cast<double2*>(dst) = make_double2(w[b][0].x - acc[0], w[b][0].y - acc[1]);
                            *reinterpret_cast<double2*>(dst + 2) = make_double2(w[b][1].x - acc[2], w[b][1].y - acc[3]);
                        }
                };
                load(wa, ta);
                for (;;) {
                    if (ta[0] < 0) break;
                    load(wb, tb);
                    update(wa, ta);
                    if (tb[0] < 0) break;
                    load(wa, ta);
                    update(wb, tb);
                }
            }
        }
        __syncthreads();
        if (p >= 0) CHOL_TS(2 + 2 * p);
    }
    if (ill) chol_ill_test(R, LP, l, d0, colflag, ill_tol, ill, &ill_s, tid, NT);
}

size_t chol_lds_bytes(int LP) {
    return (size_t)512 * 8 + (size_t)LP * 8 + (size_t)16 * (LP + kCholPad) * 8 + 256 * 8 + 32 * 4 + 64;
}

// ------------------------------------------------------------------------------------------------
// Register-resident Cholesky (LP <= 256).  chol_wide_kernel keeps the Gram being reduced in global
// memory (L2), so every block step pays two L2 round trips per tile on top of its barriers
// (10 us per 16-column step at LP = 256).  Here the upper block triangle of G lives in the
// REGISTERS of one 512-thread workgroup: upper-triangle tile t (row-major order) belongs to wave
// t % 8, slot t / 8, in MFMA output layout (lane (r, h): rows h + 4 j, column r) -- LP = 256 is 136
// tiles, 17 slots = 136 VGPRs per lane.  Row-major dealing spreads every tile row over consecutive
// waves, so the trailing triangle of each step is balanced to one tile per row.  Per block step p:
//   (A) the owner of tile (p, p) factors it (16x16 upper Cholesky + inverse, lane j owning column j),
//       D^-1 to LDS;                                                              -- barrier
//   (B) the owners of row p form the strip R[p][jb] = D_p^-T W[p][jb] (4 MFMAs), to R and to LDS;
//                                                                                 -- barrier
//   (C) every wave updates its trailing tiles W[ib][jb] -= R[p][ib]^T R[p][jb] from the LDS strip.
// (C) of step p and (A) of step p + 1 touch only the owner's registers, so two barriers per step.
// Same operations in the same order as chol_wide_kernel: bit-identical R.
constexpr int kCholRegWaves = 8;

template <int NP> struct CholReg {
    static constexpr int LP = 16 * NP, NW = kCholRegWaves, NT = NP * (NP + 1) / 2, S = (NT + NW - 1) / NW;
    // the first SL slots of every wave (rows retired earliest) live in LDS: VGPR budget at 2 waves/SIMD
    static constexpr int SL = S > 10 ? S - 10 : 0;
    static constexpr int LDR = LP + kCholPad;
    static constexpr size_t lds_bytes = (size_t)(512 + 256 + LP + 16 * LDR + NW * SL * 256) * 8 + 32 * 4;
};

// R^-1 inside the factor's own launch (round 5; NP <= 8, every leaf of the two- and three-level
// factors): the products of rinv_wide_kernel in the same order, bit-identical, but one WAVE per
// 16-column block column jb instead of one workgroup.  X[k] never leaves the wave -- its MFMA output
// layout (row h + 4 j, column r) is the B operand (rows 4 kk + h) of the next product -- so the steps
// need no workgroup barrier, and R's upper block triangle (diagonal slots: D^-1 from Rinv) is staged
// once in LDS in A-operand order (tile t of the triangle at img + 256 t, lane L's four k-values
// contiguous).  Saves the rinv_wide launch (~14 us per leaf) for ~4 us here.
template <int NP> struct CholRegInv {
    static constexpr int NT = NP * (NP + 1) / 2, NTH = 64 * kCholRegWaves;
    static constexpr int NE = (NT * 256 + NTH - 1) / NTH;  // staged doubles per thread
    static constexpr size_t lds_bytes = (size_t)NT * 256 * 8;
};
__device__ __forceinline__ int tri_index(int p, int k, int np) { return p * np - p * (p - 1) / 2 + (k - p); }

// Below the block diagonal of an LP x LP factor: zeros in R, Rinv, Rinv32 (row-major) and the pieces
// (transposed), each array walked in its own layout so every store instruction is contiguous.
__device__ __forceinline__ void chol_lower_zeros(int LP, double* __restrict__ R, double* __restrict__ Rinv,
                                                 float* __restrict__ Rinv32, bf16_t* __restrict__ Mt, int t0,
                                                 int nthr) {
    const int64_t L2 = (int64_t)LP * LP;
    for (int e = t0; e < LP * LP; e += nthr) {
        const int a = e / LP, b = e % LP;
        if (a >= 16 * (b / 16 + 1)) {  // row a, column b
            R[e] = 0.0;
            Rinv[e] = 0.0;
            if (Rinv32) Rinv32[e] = 0.0f;
        }
        if (Mt && b >= 16 * (a / 16 + 1)) {  // column a, row b
            Mt[e] = 0;
            Mt[L2 + e] = 0;
            Mt[2 * L2 + e] = 0;
        }
    }
}

template <int NP>
__device__ __forceinline__ void chol_reg_rinv(double* __restrict__ img, double* __restrict__ R,
                                              double* __restrict__ Rinv, float* __restrict__ Rinv32,
                                              bf16_t* __restrict__ Mt, int tid, int wv, int lane) {
    typedef CholRegInv<NP> C;
    constexpr int LP = 16 * NP;
    const int64_t L2 = (int64_t)LP * LP;
    const int r = lane & 15, h = lane >> 4;
    __syncthreads();  // the factor's LDS is dead; its R / Rinv stores are visible workgroup-wide
    {
        // the full NP x NP tile grid, upper triangle kept: shifts only, every load issued before any store
        constexpr int NF = NP * NP * 256 / C::NTH;
        double v[NF];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int e = tid + i * C::NTH;
            const int t2 = e >> 8, p = t2 / NP, k = t2 % NP, L = (e >> 2) & 63, kk = e & 3;
            const int64_t src = (int64_t)(16 * p + (L & 15)) * LP + 16 * k + 4 * kk + (L >> 4);
            v[i] = 0.0;
            if (p < k) v[i] = R[src];
            else if (p == k) v[i] = Rinv[src];
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int e = tid + i * C::NTH;
            const int t2 = e >> 8, p = t2 / NP, k = t2 % NP;
            if (p <= k) img[tri_index(p, k, NP) * 256 + (e & 255)] = v[i];
        }
    }
    __syncthreads();
    CHOL_TS(210);
    // column jb's 2 jb^2 + 6 jb MFMAs: waves w and w + 4 share a SIMD, so pair the long columns with
    // the short ones (NP = 8: 7 + 0, 6 + 1, 5 + 2, 4 + 3; 140 MFMAs on the busiest SIMD instead of 176)
    const int jb = NP == 8 ? (wv < 4 ? 7 - wv : wv - 4) : wv, c0 = 16 * jb;
    if (jb >= NP) return;
    f64x4 T[NP];
#pragma unroll
    for (int s = 0; s < NP; ++s) T[s] = MD::zero();
    for (int k = jb; k >= 0; --k) {
        const double* dk = img + tri_index(k, k, NP) * 256;
        f64x4 x;
        if (k == jb) {  // D_jb^-1 in output layout: element (h + 4 j, r) sits in lane (h + 4 j) + 16 (r & 3), slot r >> 2
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = dk[((h + 4 * j) + 16 * (r & 3)) * 4 + (r >> 2)];
        } else {
            f64x4 t = MD::zero();
#pragma unroll
            for (int s = 0; s < NP; ++s)
                if (s == k) t = T[s];
            const double2 d01 = *reinterpret_cast<const double2*>(dk + lane * 4);
            const double2 d23 = *reinterpret_cast<const double2*>(dk + lane * 4 + 2);
            f64x4 o = MD::zero();
            o = MD::mma(d01.x, t[0], o);
            o = MD::mma(d01.y, t[1], o);
            o = MD::mma(d23.x, t[2], o);
            o = MD::mma(d23.y, t[3], o);
#pragma unroll
            for (int j = 0; j < 4; ++j) x[j] = -o[j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = h + 4 * j;
            if (k != jb) Rinv[(int64_t)(16 * k + i) * LP + c0 + r] = x[j];
            if (Rinv32) Rinv32[(int64_t)(16 * k + i) * LP + c0 + r] = (float)x[j];
            if (Mt) store_pieces(Mt, L2, (int64_t)(c0 + r) * LP + 16 * k + i, (float)x[j]);
        }
#pragma unroll
        for (int s = NP - 1; s >= 0; --s)  // T[k - 1] first: the next step's product waits on it
            if (s < k) {
                const double* a = img + tri_index(s, k, NP) * 256 + lane * 4;
                const double2 a01 = *reinterpret_cast<const double2*>(a);
                const double2 a23 = *reinterpret_cast<const double2*>(a + 2);
                T[s] = MD::mma(a01.x, x[0], T[s]);
                T[s] = MD::mma(a01.y, x[1], T[s]);
                T[s] = MD::mma(a23.x, x[2], T[s]);
                T[s] = MD::mma(a23.y, x[3], T[s]);
            }
    }
#ifdef RSVD_CHOL_PROF
    if (lane == 0) g_chol_prof[211 + jb] = wall_clock64();
#endif
    // the zeros below the block diagonal: on the waves of the short columns, after their column
    if (2 * jb < NP) chol_lower_zeros(LP, R, Rinv, Rinv32, Mt, jb * 64 + lane, NP / 2 * 64);
}

template <int NP>
__global__ __launch_bounds__(64 * kCholRegWaves) void chol_reg_kernel(const double* __restrict__ G, int l, double tol,
                                                                      double* __restrict__ R, double* __restrict__ Rinv,
                                                                      int* __restrict__ colflag, int* __restrict__ flag,
                                                                      const int* __restrict__ pred, double ill_tol,
                                                                      int* __restrict__ ill, const double* __restrict__ d0src,
                                                                      int ldg, float* __restrict__ Rinv32,
                                                                      bf16_t* __restrict__ Mt, int fuse_rinv) {
    if (pred && *pred == 0) return;
    typedef CholReg<NP> C;
    __shared__ int ill_s;
    constexpr int LP = C::LP, NW = C::NW, NT = C::NT, S = C::S, SL = C::SL, LDR = C::LDR;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* Di = reinterpret_cast<double*>(smem_raw);  // [2][256]
    double* Tsc = Di + 512;                            // [256]
    double* d0 = Tsc + 256;                            // [LP]
    double* Rs = d0 + LP;                              // [16][LDR]
    double* wl = Rs + 16 * LDR;                        // [NW][SL][64 lanes][4]
    int* bad = reinterpret_cast<int*>(wl + NW * SL * 256);  // [2][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, h = lane >> 4;
    double* wlw = wl + wv * SL * 256 + lane * 4;
    CHOL_TS(97);

    int tib[S], tjb[S];
    double wt[S - SL > 0 ? S - SL : 1][4];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        tib[s] = NP;  // empty slot: never active
        tjb[s] = NP;
        const int t = s * NW + wv;
        if (t < NT) tri_decode(t, NP, tib[s], tjb[s]);
        double v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = 16 * tib[s] + h + 4 * j, c = 16 * tjb[s] + r;
            v[j] = (t < NT && i < l && c < l) ? G[(int64_t)i * ldg + c] : 0.0;
        }
        if (s < SL) {
            *reinterpret_cast<double2*>(wlw + s * 256) = make_double2(v[0], v[1]);
            *reinterpret_cast<double2*>(wlw + s * 256 + 2) = make_double2(v[2], v[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) wt[s < SL ? 0 : s - SL][j] = v[j];
        }
    }
    auto get = [&](int s, double (&v)[4]) {
        if (s < SL) {
            const double2 a = *reinterpret_cast<const double2*>(wlw + s * 256);
            const double2 b = *reinterpret_cast<const double2*>(wlw + s * 256 + 2);
            v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = wt[s < SL ? 0 : s - SL][j];
        }
    };
    for (int i = tid; i < LP; i += 64 * NW) {
        d0[i] = (i < l) ? (d0src ? d0src[i] : G[(int64_t)i * ldg + i]) : 0.0;
        colflag[i] = 0;
    }
    if (tid == 0) ill_s = 0;
    __syncthreads();
    CHOL_TS(200);

    for (int p = 0; p < NP; ++p) {
        const int p16 = 16 * p;
        // (A) factor the diagonal tile (p, p) on its owner wave
        const int tpp = p * NP - p * (p - 1) / 2;
        if (wv == tpp % NW) {
            const int sp = tpp / NW;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (s == sp) {
                    double v[4];
                    get(s, v);
#pragma unroll
                    for (int j = 0; j < 4; ++j) Tsc[(h + 4 * j) * 16 + r] = v[j];
                }
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            double col[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) col[i] = Tsc[i * 16 + r];
            __builtin_amdgcn_s_waitcnt(0xc07f);
            __builtin_amdgcn_wave_barrier();
            chol_diag16_v2(col, p16, l, LP, tol, d0, Di + (p & 1) * 256, bad + (p & 1) * 16, R, Rinv,
                           colflag, flag, lane, Tsc);
        }
        __syncthreads();
        if (p < 32) CHOL_TS(1 + 3 * p);
        if (p == NP - 1) {
            if (ill) chol_ill_test(R, LP, l, d0, colflag, ill_tol, ill, &ill_s, tid, 64 * NW);
            break;
        }
        // (B) strip R[p][jb] = D_p^-T W[p][jb] (0 for rows that broke down or are padding)
        {
            const double* Dp = Di + (p & 1) * 256;
            const int* bd = bad + (p & 1) * 16;
            double x[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) x[kk] = Dp[(4 * kk + h) * 16 + r];
            int zero_rows = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) zero_rows |= (bd[h + 4 * j] || p16 + h + 4 * j >= l) << j;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (tib[s] == p && tjb[s] > p) {
                    double v[4];
                    get(s, v);
                    f64x4 acc = MD::zero();
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) acc = MD::mma(x[kk], v[kk], acc);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int i = h + 4 * j;
                        const double o = ((zero_rows >> j) & 1) ? 0.0 : acc[j];
                        R[(int64_t)(p16 + i) * LP + 16 * tjb[s] + r] = o;
                        Rs[i * LDR + 16 * tjb[s] + r] = o;
                    }
                }
        }
        __syncthreads();
        if (p < 32) CHOL_TS(2 + 3 * p);
        // (C) trailing update of the tiles below row p
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (tib[s] > p && tib[s] < NP) {
                f64x4 acc = MD::zero();
#pragma unroll
                for (int kk = 0; kk < 4; ++kk)
                    acc = MD::mma(Rs[(4 * kk + h) * LDR + 16 * tib[s] + r], Rs[(4 * kk + h) * LDR + 16 * tjb[s] + r], acc);
                if (s < SL) {
                    double v[4];
                    get(s, v);
                    *reinterpret_cast<double2*>(wlw + s * 256) = make_double2(v[0] - acc[0], v[1] - acc[1]);
                    *reinterpret_cast<double2*>(wlw + s * 256 + 2) = make_double2(v[2] - acc[2], v[3] - acc[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) wt[s < SL ? 0 : s - SL][j] -= acc[j];
                }
            }
        if (p < 32) CHOL_TS(3 + 3 * p);
    }
    if constexpr (NP <= 8) {
        if (fuse_rinv) chol_reg_rinv<NP>(reinterpret_cast<double*>(smem_raw), R, Rinv, Rinv32, Mt, tid, wv, lane);
    }
}

// R^-1 = blocked back substitution, one workgroup (4 waves) per 16-column block jb, all block
// columns in parallel:  X[jb] = D_jb^-1,  X[p] = -D_p^-1 T[p],  T[p] = sum_{p<k<=jb} R[p][k] X[k].
// Right-looking: as soon as X[k] is known every wave adds R[p][k] X[k] to the accumulators T[p] it
// owns (p = wave + 4 s, in registers), so each step is one MFMA group per owned block, one 16x16
// product on the owner wave and ONE barrier (X double-buffered in LDS); the R tiles of the next step are loaded a step ahead.
// (An accumulator in MFMA output layout -- row h + 4 j, column r in lane (r, h) -- is already the
// B operand of the next product: rows 4 kk + h.)  Also: zeros below the block diagonal of R and
// R^-1, and the fp32 copy of this block column of R^-1.
constexpr int kRinvSlots = 8;  // LP <= 512: 32 block rows over 4 waves

__global__ __launch_bounds__(256) void rinv_wide_kernel(int LP, double* __restrict__ R, double* __restrict__ Rinv,
                                                        float* __restrict__ Rinv32, const int* __restrict__ pred,
                                                        bf16_t* __restrict__ Mt) {
    const int64_t L2 = (int64_t)LP * LP;
    if (pred && *pred == 0) return;
    __shared__ double Xs[2][256];  // X[k] of the current step (buffer k & 1), row-major
    const int jb = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int r = lane & 15, h = lane >> 4;
    const int c0 = 16 * jb;
    // below the block diagonal: zeros
    for (int e = tid; e < (LP - c0 - 16) * 16; e += 256) {
        const int i = c0 + 16 + e / 16, c = c0 + e % 16;
        R[(int64_t)i * LP + c] = 0.0;
        Rinv[(int64_t)i * LP + c] = 0.0;
        if (Rinv32) Rinv32[(int64_t)i * LP + c] = 0.0f;
        if (Mt) store_pieces(Mt, L2, (int64_t)c * LP + i, 0.0f);
    }
    f64x4 T[kRinvSlots];
    double Rc[kRinvSlots][4], Rn[kRinvSlots][4], Dn[4];
#pragma unroll
    for (int s = 0; s < kRinvSlots; ++s) T[s] = MD::zero();
    // R[p][k] A-operands (row r, column 4 kk + h) of the step k for the blocks p < k this wave owns
    auto load_r = [&](double (&dst)[kRinvSlots][4], int k) {
#pragma unroll
        for (int s = 0; s < kRinvSlots; ++s) {
            const int p = wv + 4 * s;
            if (p < k) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) dst[s][kk] = R[(int64_t)(16 * p + r) * LP + 16 * k + 4 * kk + h];
            }
        }
    };
    // D_k^-1 as the A operand (row r, column 4 kk + h), loaded one owned step ahead
    auto load_d = [&](int k) {
        if (k >= 0) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) Dn[kk] = Rinv[(int64_t)(16 * k + r) * LP + 16 * k + 4 * kk + h];
        }
    };
    {
        int k1 = jb - 1;
        while (k1 >= 0 && (k1 & 3) != wv) --k1;
        load_d(k1);
    }
    load_r(Rc, jb);
    for (int k = jb; k >= 0; --k) {
        const int own = k & 3;
        if (k > 0) load_r(Rn, k - 1);
        if (wv == own) {
            f64x4 x;
            if (k == jb) {
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = Rinv[(int64_t)(c0 + h + 4 * j) * LP + c0 + r];
            } else {
                f64x4 t = MD::zero();
#pragma unroll
                for (int s = 0; s < kRinvSlots; ++s)
                    if (wv + 4 * s == k) t = T[s];
                f64x4 o = MD::zero();
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) o = MD::mma(Dn[kk], t[kk], o);
#pragma unroll
                for (int j = 0; j < 4; ++j) x[j] = -o[j];
                load_d(k - 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = h + 4 * j;
                Xs[k & 1][i * 16 + r] = x[j];
                if (k != jb) Rinv[(int64_t)(16 * k + i) * LP + c0 + r] = x[j];
                if (Rinv32) Rinv32[(int64_t)(16 * k + i) * LP + c0 + r] = (float)x[j];
                if (Mt) store_pieces(Mt, L2, (int64_t)(c0 + r) * LP + 16 * k + i, (float)x[j]);
            }
        }
        __syncthreads();
        if (k > 0) {
            double xb[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) xb[kk] = Xs[k & 1][(4 * kk + h) * 16 + r];
#pragma unroll
            for (int s = 0; s < kRinvSlots; ++s) {
                const int p = wv + 4 * s;
                if (p < k) {
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) T[s] = MD::mma(Rc[s][kk], xb[kk], T[s]);
                }
            }
#pragma unroll
            for (int s = 0; s < kRinvSlots; ++s)
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) Rc[s][kk] = Rn[s][kk];
        }
    }
}

}  // namespace

// The one-workgroup factor (+ rinv_wide_kernel where the factor's own launch does not form R^-1).
static hipError_t chol_one(const CholArgs& a, hipStream_t s) {
    const int LP = a.LP, ldg = a.ldg ? a.ldg : LP;
    if (LP % 16 || LP > 512) return hipErrorInvalidValue;
    // LP = 256: chol_wide_kernel (its wave-0 look-ahead overlaps the diagonal factor with the other waves'
    // updates; the register-resident kernel spills there, 174 vs 161 us measured); LP <= 128: chol_reg_kernel
    // (LP = 128: 63 vs 71 us, LP = 64: 31 vs 37 us, tools/wide_lab chol)
    // R^-1 by the triangular inverse in the same launch after the register-resident factor (round 6 tried
    // eliminating [G | I] in the factor's own sweep instead: 256 VGPRs + 112 B/lane scratch at NP = 8,
    // +6 us per launch measured; DESIGN.md §9c dead end 17)
    const int fuse = (a.lab_variant >= 1 && (LP == 128 || LP == 64)) ? 1 : 0;
    auto reg = [&](auto npc) {
        constexpr int NP = decltype(npc)::value;
        hipLaunchKernelGGL(chol_reg_kernel<NP>, dim3(1), dim3(64 * kCholRegWaves),
                           std::max(CholReg<NP>::lds_bytes, fuse ? CholRegInv<NP>::lds_bytes : 0), s, a.G, a.l, a.tol,
                           a.R, a.Rinv, a.colflag, a.flag, a.pred, a.ill_tol, a.ill, a.d0src, ldg, a.Rinv32, a.Mt, fuse);
    };
    if (fuse && LP == 128) reg(std::integral_constant<int, 8>{});
    else if (fuse) reg(std::integral_constant<int, 4>{});
#ifdef RSVD_LAB
    else if (a.lab_variant == 2 && LP == 256)  // the lab's register-resident LP = 256 factor (it spills)
        reg(std::integral_constant<int, 16>{});
#endif
    else
        hipLaunchKernelGGL((chol_wide_kernel<kCholThreads, kCholBatch>), dim3(1), dim3(kCholThreads), chol_lds_bytes(LP),
                           s, a.G, a.l, LP, a.tol, a.work, a.R, a.Rinv, a.colflag, a.flag, a.pred, a.ill_tol, a.ill,
                           a.d0src, ldg);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || fuse) return e;
    hipLaunchKernelGGL(rinv_wide_kernel, dim3(LP / 16), dim3(256), 0, s, LP, a.R, a.Rinv, a.Rinv32, a.pred, a.Mt);
    return hipGetLastError();
}

// ---- two-level factor, LP = 2 B (launch_chol with depth >= 0) -------------------------------------
// The levels read G11 and G22 in place (row pitch ldg); d0b = diag(G22), written by the S product's
// diagonal tiles: the breakdown / ill tests of the second level judge S's pivots against G's own
// diagonal, as the one-level factor does (d0src: that diagonal when this factor is itself a level).

// R / Rinv (2B x 2B row-major) from the level blocks; Rinv32 the fp32 copy; ill = ill1 | ill2.
// Run by extra workgroups of the Rinv12 GEMM (gemmsq_f64_kernel with a Chol2Asm job, round 5: one
// launch fewer per two-level block); the GEMM's own workgroups write Rinv12's fp32 copy and pieces.
struct Chol2Asm {
    const double* R11;
    const double* Ri11;
    const double* R22;
    const double* Ri22;
    int B;  // 0: no assembly job
    double* R;
    double* Rinv;
    float* Rinv32;
    const int* ill2;
    int* ill;
    bf16_t* Mt;
};
// element (row i of 2B, column c of B): columns c (and c + B for i >= B) of row i
__device__ __forceinline__ void chol2_assemble_elem(const Chol2Asm& a, int i, int c) {
    const int B = a.B;
    const int64_t o = (int64_t)i * 2 * B, L2 = (int64_t)4 * B * B;
    if (i < B) {
        a.R[o + c] = a.R11[i * B + c];
        a.Rinv[o + c] = a.Ri11[i * B + c];
        if (a.Rinv32) a.Rinv32[o + c] = (float)a.Ri11[i * B + c];
        if (a.Mt) store_pieces(a.Mt, L2, (int64_t)c * 2 * B + i, (float)a.Ri11[i * B + c]);
    } else {
        const int i2 = i - B;
        a.R[o + c] = 0.0;
        a.Rinv[o + c] = 0.0;
        a.R[o + B + c] = a.R22[i2 * B + c];
        a.Rinv[o + B + c] = a.Ri22[i2 * B + c];
        if (a.Rinv32) {
            a.Rinv32[o + c] = 0.f;
            a.Rinv32[o + B + c] = (float)a.Ri22[i2 * B + c];
        }
        if (a.Mt) {
            store_pieces(a.Mt, L2, (int64_t)c * 2 * B + i, 0.0f);
            store_pieces(a.Mt, L2, (int64_t)(B + c) * 2 * B + i, (float)a.Ri22[i2 * B + c]);
        }
    }
    if (a.ill && i == 0 && c == 0 && *a.ill2) *a.ill = 1;
}

// row-major C (N x N, ldc) = alpha op(A) B + beta C, N = K in {128, 256} (op(A) = A or A^T; A, B
// row-major with ld lda / ldb): one wave per 16 x 16 output tile ((N / 16)^2 workgroups -- the
// 64 x 64-tile general GEMM kept 16 CUs busy, 56 us per 256^3 product), four independent fp64 MFMA
// chains over K, every operand an L2 hit.
// K is split over the workgroup's four waves (a quarter each, four chains per wave: the one-wave form
// was a 16-deep dependent MFMA chain per accumulator behind L2 loads, 24 us per 256^3 product); the
// wave partials are summed through LDS in wave order.
constexpr int kGemmSqWaves = 4;
// zrow (nullable): output rows i with zrow[i] != 0 are written as zeros (R12's broken-down rows).
// Cin (nullable): the beta term's C when it is not the output (ld ldcin); d0out (nullable): the
// diagonal-tile workgroups also write d0out[i] = d0in ? d0in[i] : Cin[i][i] (a level's pivot reference)
struct GemmSqJob {
    int N = 0, ta = 0;  // N = 0: no job
    double alpha = 1.0;
    const double* A = nullptr;
    int lda = 0;
    const double* B = nullptr;
    int ldb = 0;
    double beta = 0.0;
    double* C = nullptr;
    int ldc = 0;
    const int* zrow = nullptr;
    const double* Cin = nullptr;
    int ldcin = 0;
    double* d0out = nullptr;
    const double* d0in = nullptr;
};
// One launch runs up to two independent products (j1.N = 0: one) and, on extra workgroups, a
// two-level factor's assembly job (round 6: the two-level factor's T = Ri11 R12 rides the S product's
// launch -- one dependent launch fewer per two-level block).
__global__ __launch_bounds__(64 * kGemmSqWaves) void gemmsq_f64_kernel(GemmSqJob j0, GemmSqJob j1, Chol2Asm aj) {
    __shared__ double part[kGemmSqWaves - 1][4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, h = lane >> 4;
    const int nb0 = (j0.N / 16) * (j0.N / 16), nb1 = (j1.N / 16) * (j1.N / 16);
    int b = (int)blockIdx.x;
    if (b >= nb0 + nb1) {  // an assembly workgroup (the Rinv12 product's launch)
        const int e = (b - nb0 - nb1) * 64 * kGemmSqWaves + (int)threadIdx.x;
        if (aj.B && e < 2 * aj.B * aj.B) chol2_assemble_elem(aj, e / aj.B, e % aj.B);
        return;
    }
    const bool second = b >= nb0;
    const GemmSqJob& J = second ? j1 : j0;
    if (second) b -= nb0;
    const int N = J.N, nt = N / 16;
    const int i0 = 16 * (b / nt), j0c = 16 * (b % nt);
    const int kq = N / kGemmSqWaves;  // N % 64 == 0
    const double* __restrict__ A = J.A;
    const double* __restrict__ B = J.B;
    const int lda = J.lda, ldb = J.ldb, ta = J.ta;
    f64x4 acc[4] = {MD::zero(), MD::zero(), MD::zero(), MD::zero()};
#pragma unroll 2
    for (int k0 = w * kq; k0 < (w + 1) * kq; k0 += 16) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + h;
            const double a = ta ? A[(int64_t)k * lda + i0 + r] : A[(int64_t)(i0 + r) * lda + k];
            acc[u] = MD::mma(a, B[(int64_t)k * ldb + j0c + r], acc[u]);
        }
    }
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
    if (w > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part[w - 1][j][lane] = v[j];
    }
    __syncthreads();
    if (w != 0) return;
    const int ldc = J.ldc;
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // f64 D: col = r, row = h + 4 j
#pragma unroll
        for (int q = 0; q < kGemmSqWaves - 1; ++q) v[j] += part[q][j][lane];
        const int ii = i0 + MD::row(h, j), jj = j0c + r;
        double* c = J.C + (int64_t)ii * ldc + jj;
        const double o = J.alpha * v[j];
        const double cin = J.beta == 0.0 ? 0.0 : (J.Cin ? J.Cin[(int64_t)ii * J.ldcin + jj] : *c);
        const double out = (J.zrow && J.zrow[ii]) ? 0.0 : (J.beta == 0.0 ? o : o + J.beta * cin);
        *c = out;
        if (J.d0out && ii == jj) J.d0out[ii] = J.d0in ? J.d0in[ii] : J.Cin[(int64_t)ii * J.ldcin + ii];
        if (!second && aj.B) {  // (the Rinv12 product: C = Rinv + B, ldc = 2 B) its fp32 copy and pieces
            if (aj.Rinv32) aj.Rinv32[(int64_t)ii * ldc + aj.B + jj] = (float)out;
            if (aj.Mt) store_pieces(aj.Mt, (int64_t)4 * aj.B * aj.B, (int64_t)(aj.B + jj) * 2 * aj.B + ii, (float)out);
        }
    }
}

static GemmSqJob sq_job(int N, int ta, double alpha, const double* A, int lda, const double* B, int ldb, double beta,
                        double* C, int ldc, const int* zrow = nullptr, const double* Cin = nullptr, int ldcin = 0,
                        double* d0out = nullptr, const double* d0in = nullptr) {
    GemmSqJob j;
    j.N = N, j.ta = ta, j.alpha = alpha, j.A = A, j.lda = lda, j.B = B, j.ldb = ldb, j.beta = beta, j.C = C, j.ldc = ldc;
    j.zrow = zrow, j.Cin = Cin, j.ldcin = ldcin, j.d0out = d0out, j.d0in = d0in;
    return j;
}

static hipError_t gemm_sq2(const GemmSqJob& j0, const GemmSqJob& j1, hipStream_t s, const Chol2Asm* aj = nullptr) {
    if (j0.N % (16 * kGemmSqWaves) || j1.N % (16 * kGemmSqWaves)) return hipErrorInvalidValue;
    Chol2Asm job{};
    int extra = 0;
    if (aj) {
        job = *aj;
        extra = (2 * job.B * job.B + 64 * kGemmSqWaves - 1) / (64 * kGemmSqWaves);
    }
    const int nb = (j0.N / 16) * (j0.N / 16) + (j1.N / 16) * (j1.N / 16) + extra;
    hipLaunchKernelGGL(gemmsq_f64_kernel, dim3(nb), dim3(64 * kGemmSqWaves), 0, s, j0, j1, job);
    return hipGetLastError();
}

static hipError_t gemm_sq(int N, int ta, double alpha, const double* A, int lda, const double* B, int ldb, double beta,
                          double* C, int ldc, hipStream_t s, const int* zrow = nullptr, const double* Cin = nullptr,
                          int ldcin = 0, double* d0out = nullptr, const double* d0in = nullptr,
                          const Chol2Asm* aj = nullptr) {
    return gemm_sq2(sq_job(N, ta, alpha, A, lda, B, ldb, beta, C, ldc, zrow, Cin, ldcin, d0out, d0in), GemmSqJob{}, s,
                    aj);
}

size_t chol_2level_scratch_doubles(int LP, int depth) {
    const size_t B = LP / 2;
    const size_t own = 7 * B * B + B + 64;  // Ga R11 Ri11 Sb R22 Ri22 T, d0b, ill2 (+ alignment)
    return own + (depth > 0 && B >= 256 ? chol_2level_scratch_doubles((int)B, depth - 1) : 0);
}

// The two-level form (its levels recursing `depth` more times) when depth >= 0, LP is 256 or 512 and more
// than half the columns are valid, else the one-workgroup kernel.
hipError_t launch_chol(const CholArgs& a, hipStream_t s) {
    if (a.depth >= 0 && a.pred) return hipErrorInvalidValue;  // the two-level form has no predicate
    const int l = a.l, LP = a.LP, ldg = a.ldg ? a.ldg : LP;
    if (a.depth < 0 || (LP != 256 && LP != 512) || l <= LP / 2) return chol_one(a, s);
    if (l > LP || !a.scratch) return hipErrorInvalidValue;
    const double *G = a.G, *d0src = a.d0src;
    double *R = a.R, *Rinv = a.Rinv;
    const int B = LP / 2, B2 = B * B;
    // (the first B2 doubles are unused since round 5: the levels read G11 and G22 in place -- no copy launch)
    double *R11 = a.scratch + B2, *Ri11 = R11 + B2, *Sb = Ri11 + B2, *R22 = Sb + B2, *Ri22 = R22 + B2, *T = Ri22 + B2,
           *d0b = T + B2;
    int* ill2 = reinterpret_cast<int*>(d0b + B);
    CholArgs lv = a;  // a level: B columns, no fp32 copy or pieces; depth < 0: a one-workgroup factor
    lv.LP = B, lv.Rinv32 = nullptr, lv.Mt = nullptr, lv.depth = a.depth - 1, lv.scratch = d0b + B + 64;
    // level 1: R11, Ri11 = chol(G11) (columns 0 .. B - 1 of colflag), G11 read in place (pitch ldg)
    lv.ldg = ldg, lv.l = B, lv.R = R11, lv.Rinv = Ri11;
    hipError_t e = launch_chol(lv, s);
    if (e != hipSuccess) return e;
    // R12 = Ri11^T G12 -> R[:B, B:] (ld LP); the rows whose first-level pivot broke down are zero, as
    // the one-level factor's strips are (written so by the product's epilogue)
    if ((e = gemm_sq(B, 1, 1.0, Ri11, B, G + B, ldg, 0.0, R + B, LP, s, a.colflag)) != hipSuccess) return e;
    // S = G22 - R12^T R12 into Sb (the beta term read from G22 in place), and d0b = diag(G22) (or the
    // caller's d0src[B ..]) from the diagonal tiles; in the same launch T = Ri11 R12 (independent of S)
    if ((e = gemm_sq2(sq_job(B, 1, -1.0, R + B, LP, R + B, LP, 1.0, Sb, B, nullptr, G + (int64_t)B * ldg + B, ldg, d0b,
                             d0src ? d0src + B : nullptr),
                      sq_job(B, 0, 1.0, Ri11, B, R + B, LP, 0.0, T, B), s)) != hipSuccess)
        return e;
    // level 2 on the l - B valid columns of S, tested against diag(G22) (or the caller's d0src)
    lv.G = Sb, lv.ldg = B, lv.l = l - B, lv.R = R22, lv.Rinv = Ri22, lv.colflag = a.colflag + B;
    lv.ill = a.ill ? ill2 : nullptr, lv.d0src = d0b;
    if ((e = launch_chol(lv, s)) != hipSuccess) return e;
    // Rinv12 = -(Ri11 R12) Ri22 -> Rinv[:B, B:], with the blocks' assembly into R / Rinv (+ Rinv32,
    // pieces, ill) on extra workgroups
    const Chol2Asm job{R11, Ri11, R22, Ri22, B, R, Rinv, a.Rinv32, ill2, a.ill, a.Mt};
    return gemm_sq(B, 0, -1.0, T, B, Ri22, B, 0.0, Rinv + B, LP, s, nullptr, nullptr, 0, nullptr, nullptr, &job);
}

}  // namespace rsvd

#ifdef RSVD_CHOL_PROF
#include <vector>
namespace rsvd {
namespace {
// one wave factors a 16 x 16 SPD tile `reps` times (the diagonal factor alone, no barriers): cycles per factor
template <int V>
__global__ __launch_bounds__(64) void diag_bench_kernel(const double* __restrict__ T, int reps, double* R, double* Rinv,
                                                        int* colflag, int* flag, long long* out) {
    __shared__ double Di[256], d0[16], Ts[256];
    __shared__ int bad[16];
    const int lane = threadIdx.x, r = lane & 15;
    if (lane < 16) d0[lane] = T[lane * 16 + lane];
    for (int e = lane; e < 256; e += 64) Ts[e] = T[e];
    __syncthreads();
    double col0[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) col0[i] = T[i * 16 + r];
    double sink = 0.0;
    const long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < reps; ++it) {
        double col[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) col[i] = col0[i] + sink * 1e-300;
        if constexpr (V == 0) chol_diag16_dpp(col, 0, 16, 16, 1e-13, d0, Di, bad, R, Rinv, colflag, flag, lane);
        else chol_diag16_v2(col, 0, 16, 16, 1e-13, d0, Di, bad, R, Rinv, colflag, flag, lane, Ts);
        sink += col[15];
    }
    const long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0) out[V] = (t1 - t0) / reps + (sink == 12345.0 ? 1 : 0);
}
}  // namespace
void chol_diag_bench() {
    std::vector<double> h(256);
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) h[i * 16 + j] = (i == j ? 20.0 : 0.0) + 1.0 / (1 + i + j);
    double *T, *R, *Ri;
    int *cf, *fl;
    long long* out;
    (void)hipMalloc(&T, 256 * 8);
    (void)hipMalloc(&R, 256 * 8);
    (void)hipMalloc(&Ri, 256 * 8);
    (void)hipMalloc(&cf, 64);
    (void)hipMalloc(&fl, 64);
    (void)hipMalloc(&out, 16);
    (void)hipMemcpy(T, h.data(), 256 * 8, hipMemcpyHostToDevice);
    long long o[2];
    std::vector<double> r1(256), r2(256), i1(256), i2(256);
    for (int rep = 0; rep < 2; ++rep) {
        hipLaunchKernelGGL(diag_bench_kernel<0>, dim3(1), dim3(64), 0, 0, T, 256, R, Ri, cf, fl, out);
        (void)hipMemcpy(r1.data(), R, 256 * 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(i1.data(), Ri, 256 * 8, hipMemcpyDeviceToHost);
        hipLaunchKernelGGL(diag_bench_kernel<1>, dim3(1), dim3(64), 0, 0, T, 256, R, Ri, cf, fl, out);
        (void)hipMemcpy(r2.data(), R, 256 * 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(i2.data(), Ri, 256 * 8, hipMemcpyDeviceToHost);
        (void)hipMemcpy(o, out, 16, hipMemcpyDeviceToHost);
    }
    printf("  16x16 diagonal factor, one wave: DPP form %lld cycles, v2 %lld cycles "
           "(v2 bit-identical to DPP: R %d, R^-1 %d)\n", o[0], o[1], (int)(r1 == r2), (int)(i1 == i2));
    (void)hipFree(T); (void)hipFree(R); (void)hipFree(Ri); (void)hipFree(cf); (void)hipFree(fl); (void)hipFree(out);
}
void chol_prof_dump(int LP, int variant) {  // variant: the CholArgs::lab_variant the timed factor ran with
    long long t[256];
    (void)hipMemcpyFromSymbol(t, HIP_SYMBOL(g_chol_prof), sizeof(t));
    const int np = LP / 16;
    double strip = 0, trail = 0;
    const double us = 0.01;  // wall_clock64 runs at 100 MHz
    long long prev = t[0];
    for (int p = 0; p < np; ++p) {
        strip += (t[1 + 2 * p] - prev) * us;
        trail += (t[2 + 2 * p] - t[1 + 2 * p]) * us;
        prev = t[2 + 2 * p];
    }
    if (variant == 0) {
        printf("  LP=%d factor phases (us): init+diag0 %.1f strip %.1f trailing+diag %.1f\n", LP, (t[0] - t[97]) * us,
               strip, trail);
        return;
    }
    double A = 0, B = 0, Cc = 0;
    prev = t[200];
    for (int p = 0; p < np && p < 32; ++p) {
        A += (t[1 + 3 * p] - prev) * us;
        if (p == np - 1) break;
        B += (t[2 + 3 * p] - t[1 + 3 * p]) * us;
        Cc += (t[3 + 3 * p] - t[2 + 3 * p]) * us;
        prev = t[3 + 3 * p];
    }
    printf("  LP=%d reg phases (us, wave 0): init %.1f  diag+wait %.1f  strip %.1f  update %.1f\n", LP,
           (t[200] - t[97]) * us, A, B, Cc);
    if (np <= 8) {
        const long long f = t[1 + 3 * (np - 1)];
        printf("  LP=%d fused R^-1 (us after the factor): staged %.2f, columns", LP, (t[210] - f) * us);
        for (int j = 0; j < np; ++j) printf(" %.2f", (t[211 + j] - f) * us);
        printf("\n");
    }
}
}  // namespace rsvd
#endif
