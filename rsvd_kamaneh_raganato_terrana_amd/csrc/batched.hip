// batched.hip -- the fused batched rSVD: the whole of src/rSVD.cpp:72-133 for one small matrix on ONE
// workgroup, one launch for a batch of matrices or for the tiles of one large matrix (the block
// decomposition of image_compression/src/image_com.cpp:350-371, one independent rSVD per block).
//
// Per matrix (m x n, max(m, n) <= 256, l <= 64), all inside the workgroup:
//   Omega (Philox(seed + b) or the caller's) -> Pn                       generateOmega     src/rSVD.cpp:81
//   Pm = A Pn ; Pm = orth(Pm)                                            intermediate_step src/rSVD.cpp:59-61
//   q x { Pn = A^T Pm ; orth ; Pm = A Pn ; orth }                                          src/rSVD.cpp:62-69
//   Pn = B^T = A^T Pm ; B^T = Q_B R (R kept, Pn = Q_B)                   B = Q^T A         src/rSVD.cpp:89
//   W = R^T = U_w S V_w^T, one-sided Jacobi in LDS (as jacobi.hip)       SVD<Jacobi>       SVD_class.hpp:126-178
//   U = Pm U_w ; V = Pn V_w                                              U = Q * Utilde    src/rSVD.cpp:128
// and, for a compress call (COMP), from the same LDS contents:
//   C = U_k diag(S_k) V_k^T over or beside A, ||A||_F^2, ||A - C||_F^2   localMatrix = U * S.asDiagonal() *
//                                             V.transpose()  image_compression/src/image_com.cpp:374, :381-394
//
// Pm (m x l) and Pn (n x l) are column-major panels in T, in LDS behind the l x l area when they fit
// in the 160 KiB budget, else in the workgroup's slice of the handle workspace.  A is read in place
// through its base pointer and lda with scalar loads (tiles of a larger matrix start anywhere).
//
// Orthonormalisation: Householder reflectors on the panel where it lies (what the reference itself
// does, src/rSVD.cpp:60-61), Q formed in place by backward accumulation.  A product of reflectors is
// orthogonal whatever the panel's rank, so a constant or zero tile needs no second code path: a zero
// column gets the identity reflector and Q's column is the completing unit vector.  Every sum (the
// projections, the reflector norms and dot products) is accumulated in fp64 in a fixed order -- lanes
// own rows, a 64-lane butterfly joins them -- and rounded to T when stored; no atomics touch data.
// The products are plain FMAs: on gfx950 the f32-input and f64 MFMAs run at the vector FMA rate, the
// operands here arrive at odd pitches, and an item per (row, 8 columns) needs no fragment shuffles.
#include "batched.hpp"
#include "common.hpp"

namespace rsvd {

namespace {

template <int CTRL>
__device__ __forceinline__ double bdpp(double v) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)u, CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(unsigned)(u >> 32), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
template <int CTRL>
__device__ __forceinline__ float bdpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// sum over an aligned group of 16 lanes (jacobi.hip group_sum<16>)
template <typename C>
__device__ __forceinline__ C sum16(C v) {
    v += bdpp<0xB1>(v);   // quad_perm [1,0,3,2]
    v += bdpp<0x4E>(v);   // quad_perm [2,3,0,1]
    v += bdpp<0x141>(v);  // row_half_mirror
    v += bdpp<0x140>(v);  // row_mirror
    return v;
}

__device__ __forceinline__ double brsqrt(double d) {
    const double y = __builtin_amdgcn_rsq(d);
    return y * (1.5 - 0.5 * d * y * y);
}
__device__ __forceinline__ float brsqrt(float d) {
    const float y = __builtin_amdgcn_rsqf(d);
    return y * (1.5f - 0.5f * d * y * y);
}
__device__ __forceinline__ double brcp(double d) {
    double y = __builtin_amdgcn_rcp(d);
    y = y * (2.0 - d * y);
    return y * (2.0 - d * y);
}
__device__ __forceinline__ float brcp(float d) {
    const float y = __builtin_amdgcn_rcpf(d);
    return y * (2.0f - d * y);
}

template <typename C> struct BEps;
template <> struct BEps<double> {
    static constexpr double eps = 2.220446049250313e-16;
    static constexpr double quad2 = 1e-16;
    static constexpr double lo = 1e-290, hi = 1e290;
    // |binary exponent| of max |W| this kernel accepts, and the range of 2^-wexp in T.  Nothing here
    // squares in T (house_factor and the projections sum in fp64), but the panels are stored in T: with
    // max |W| at 2^-56 an entry 2^-70 below it is T = float's last normal number, and above 2^56 the
    // rebuilt C and its squares leave little headroom.  Kept equal to jacobi.hip's Eps<>::emax so that
    // both fp32 paths report the same window (rsvd_c.h); outside it the matrix is marked non-finite.
    static constexpr int emax = 480, eclamp = 1000;
};
template <> struct BEps<float> {
    static constexpr double eps = 1.1920928955078125e-07;
    static constexpr double quad2 = 1e-8;
    static constexpr double lo = 1e-35, hi = 1e35;
    static constexpr int emax = 56, eclamp = 120;
};

// Thread and LDS layout of the l x l area.  The Jacobi rounds use 16 threads per column pair as
// jacobi.hip; the projections and reflectors use every thread of the workgroup.
template <typename T, int LP>
struct BShape {
    static constexpr int TPP = 16;
    static constexpr int CH = LP / TPP;                      // rows per thread of a pair
    static constexpr int CS = LP + 16 / (int)sizeof(T);      // Jacobi column stride (staggered banks)
    static constexpr int NJ = (LP / 2) * TPP;
    static constexpr int NT = NJ > 256 ? NJ : 256;           // workgroup size
    static constexpr size_t oX = 0;                                         // [LP][CS] T   rotated columns
    static constexpr size_t oJ = oX + (size_t)LP * CS * sizeof(T);          // [LP][CS] T   accumulated rotations
    static constexpr size_t oUd = oJ + (size_t)LP * CS * sizeof(T);         // [LP][LP] f64 U_w, column k contiguous
    static constexpr size_t oSig = oUd + (size_t)LP * LP * sizeof(double);  // [LP] f64
    static constexpr size_t oV = oSig + LP * sizeof(double);                // [LP] f64 scratch
    static constexpr size_t oNrm = oV + LP * sizeof(double);                // [LP] T (8-byte slots)
    static constexpr size_t oTau = oNrm + LP * sizeof(double);              // [LP] f64 reflector scalars
    static constexpr size_t oRank = oTau + LP * sizeof(double);             // [LP] int
    static constexpr size_t oFlags = oRank + LP * sizeof(int);              // [8] int
    static constexpr size_t bytes = (oFlags + 8 * sizeof(int) + 15) & ~size_t(15);
};

// flags[]: 0, 1 Jacobi sweep state; 2 completion candidate; 3 a reflector met a numerically zero
// column; 4 non-finite R or S, or W outside the accepted range; 5 the biased binary exponent of the
// largest |W| entry (0: W is zero).
constexpr int kFlDeficient = 3, kFlNonFinite = 4, kFlWexp = 5;

// 2^e for |e| <= 1022, assembled from its exponent field, and the e of |x| = f 2^e, f in [0.5, 1)
__device__ __forceinline__ double pow2(int e) {
    return __builtin_bit_cast(double, (unsigned long long)(unsigned)(1023 + e) << 52);
}
__device__ __forceinline__ int frexp_exp(double x) { return __builtin_amdgcn_frexp_exp(x); }
__device__ __forceinline__ int frexp_exp(float x) { return __builtin_amdgcn_frexp_expf(x); }

// The binary exponent W is divided by, from flags[kFlWexp], clamped to the range of 2^-wexp in T.
template <typename T>
__device__ __forceinline__ int wexp_of(const int* flags) {
    const int w = flags[kFlWexp] ? flags[kFlWexp] - 2048 : 0;
    return w > BEps<T>::eclamp ? BEps<T>::eclamp : (w < -BEps<T>::eclamp ? -BEps<T>::eclamp : w);
}

// Out (rows x cols, column-major ldo; column colmap[c] when given) = scale * A (rows x K, column-major
// lda) * X (K x cols, column-major ldx).  One item = one row and 8 columns; the K sum runs in order.
template <typename TA, typename TX, typename TO>
__device__ void gemm_nn(const TA* A, int64_t lda, int rows, int K, const TX* X, int ldx, int cols, TO* Out,
                        int64_t ldo, const int* colmap, double scale) {
    const int nch = (cols + 7) / 8;
    for (int it = threadIdx.x; it < rows * nch; it += blockDim.x) {
        const int i = it % rows, c0 = (it / rows) * 8;
        double acc[8];
        int cc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            acc[c] = 0.0;
            cc[c] = (c0 + c < cols ? c0 + c : cols - 1) * ldx;  // clamped: the extra sums are dropped
        }
        const TA* ap = A + i;
        for (int j = 0; j < K; ++j) {
            const double av = (double)ap[(int64_t)j * lda];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fma(av, (double)X[j + cc[c]], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c0 + c < cols) Out[i + (int64_t)(colmap ? colmap[c0 + c] : c0 + c) * ldo] = (TO)(acc[c] * scale);
    }
}

// Out (n x cols, column-major ldo) = A^T (A m x n, column-major lda) * Q (m x cols, column-major ldq).
template <typename T>
__device__ void gemm_tn(const T* A, int64_t lda, int m, int n, const T* Q, int ldq, int cols, T* Out, int ldo) {
    const int nch = (cols + 7) / 8;
    for (int it = threadIdx.x; it < n * nch; it += blockDim.x) {
        const int j = it % n, c0 = (it / n) * 8;
        double acc[8];
        int cc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            acc[c] = 0.0;
            cc[c] = (c0 + c < cols ? c0 + c : cols - 1) * ldq;
        }
        const T* ap = A + (int64_t)j * lda;
        for (int i = 0; i < m; ++i) {
            const double av = (double)ap[i];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fma(av, (double)Q[i + cc[c]], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (c0 + c < cols) Out[j + (c0 + c) * ldo] = (T)acc[c];
    }
}

// Householder QR of the column-major r x l panel P (ld r), in place: R on and above the diagonal, the
// reflector vectors (v_k = 1 implied) below it, their scalars in tau (LAPACK geqr2's layout).  A
// column with nothing below its diagonal, or none of it finite, keeps the identity reflector.
// cn: l fp64 words of scratch.  flags[kFlDeficient] is raised when what a reflector has left to work
// on lies below 1024 eps of the panel's largest column: the sketch is numerically rank-deficient.
template <typename T>
__device__ void house_factor(T* P, int r, int l, double* tau, double* cn, int* flags) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int c = wave; c < l; c += nw) {
        double s = 0.0;
        for (int i = lane; i < r; i += 64) {
            const double x = (double)P[i + c * r];
            s = fma(x, x, s);
        }
        s = warp_sum(s);
        if (lane == 0) cn[c] = s;
    }
    __syncthreads();
    double mx = 0.0;
    for (int c = 0; c < l; ++c) mx = fmax(mx, cn[c]);
    constexpr double thr = 1024.0 * BEps<T>::eps;
    const double small2 = thr * thr * mx;
    for (int k = 0; k < l; ++k) {
        if (wave == 0) {
            T* col = P + k * r;
            double s2 = 0.0;
            for (int i = k + 1 + lane; i < r; i += 64) {
                const double x = (double)col[i];
                s2 = fma(x, x, s2);
            }
            s2 = warp_sum(s2);
            const double alpha = (double)col[k];
            const double n2 = fma(alpha, alpha, s2);
            double t = 0.0, beta = alpha, inv = 0.0;
            if (s2 > 0.0 && isfinite(n2)) {
                const double nrm = sqrt(n2);
                beta = alpha >= 0.0 ? -nrm : nrm;
                t = (beta - alpha) / beta;
                inv = 1.0 / (alpha - beta);
            }
            for (int i = k + 1 + lane; i < r; i += 64) col[i] = (T)((double)col[i] * inv);
            if (lane == 0) {
                col[k] = (T)beta;
                tau[k] = t;
                if (!(n2 > small2)) flags[kFlDeficient] = 1;
            }
        }
        __syncthreads();
        const double t = tau[k];
        if (t != 0.0) {
            const T* v = P + k * r;
            for (int c = k + 1 + wave; c < l; c += nw) {
                T* col = P + c * r;
                double w = lane == 0 ? (double)col[k] : 0.0;
                for (int i = k + 1 + lane; i < r; i += 64) w = fma((double)v[i], (double)col[i], w);
                w = warp_sum(w) * t;
                for (int i = k + 1 + lane; i < r; i += 64) col[i] = (T)fma(-w, (double)v[i], (double)col[i]);
                if (lane == 0) col[k] = (T)((double)col[k] - w);
            }
        }
        __syncthreads();
    }
}

// The first l columns of Q = H_0 H_1 .. H_{l-1}, over the factored panel (LAPACK org2r).
template <typename T>
__device__ void house_form_q(T* P, int r, int l, const double* tau) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int k = l - 1; k >= 0; --k) {
        const double t = tau[k];
        const T* v = P + k * r;
        if (t != 0.0) {
            for (int c = k + 1 + wave; c < l; c += nw) {
                T* col = P + c * r;
                double w = lane == 0 ? (double)col[k] : 0.0;
                for (int i = k + 1 + lane; i < r; i += 64) w = fma((double)v[i], (double)col[i], w);
                w = warp_sum(w) * t;
                for (int i = k + 1 + lane; i < r; i += 64) col[i] = (T)fma(-w, (double)v[i], (double)col[i]);
                if (lane == 0) col[k] = (T)((double)col[k] - w);
            }
        }
        __syncthreads();
        T* col = P + k * r;
        for (int i = tid; i < r; i += blockDim.x)
            col[i] = i < k ? T(0) : (i == k ? (T)(1.0 - t) : (T)(-t * (double)col[i]));
        __syncthreads();
    }
}

__device__ __forceinline__ void brr_pair(int round, int k, int N, int& p, int& q) {
    if (k == 0) {
        p = round;
        q = N - 1;
    } else {
        p = round + k;
        p -= (p >= N - 1) ? N - 1 : 0;
        q = round - k + (N - 1);
        q -= (q >= N - 1) ? N - 1 : 0;
    }
}

// One-sided Jacobi on the columns of X (LP x LP in LDS, the l x l W / 2^wexp in its corner -- the
// caller's exact scaling, as jacobi.hip -- and J = I), round-robin pair order, the rotation and
// stopping rules of jacobi.hip.  Leaves the rotated columns in X, the accumulated rotations in J, sig
// (of the scaled W; 0 for negligible or non-finite columns) and the descending rank of every column.
// Returns the sweeps.
template <typename C, int LP>
__device__ __forceinline__ int jacobi_lds(char* sm, int l) {
    typedef BShape<C, LP> SH;
    constexpr int TPP = SH::TPP, CH = SH::CH, CS = SH::CS;
    C* X = reinterpret_cast<C*>(sm + SH::oX);
    C* J = reinterpret_cast<C*>(sm + SH::oJ);
    double* sig = reinterpret_cast<double*>(sm + SH::oSig);
    C* nrm = reinterpret_cast<C*>(sm + SH::oNrm);
    int* rank = reinterpret_cast<int*>(sm + SH::oRank);
    int* flags = reinterpret_cast<int*>(sm + SH::oFlags);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int N = (l & 1) ? l + 1 : l;  // a dummy zero column when l is odd (l < LP then)
    const int npairs = N / 2;
    const int pi = tid / TPP, sub = tid % TPP;
    const bool active = pi < npairs;
    // A pair rotates while |<x_p, x_q>| > 2 eps |x_p| |x_q| (jacobi.hip stops at l eps): the pairs left
    // alone bound ||U_w^T U_w - I||_F by l * tol, which at l = 64 in fp32 must stay well under 1e-4.
    const C tol = (C)(2.0 * BEps<C>::eps);
    const C tol2 = tol * tol;
    int sweeps = 0;
    C negl = C(0);
    for (; sweeps < 40; ++sweeps) {
        if (sweeps == 0)
            for (int c = tid; c < LP; c += nt) {
                C s2 = C(0);
                for (int i = 0; i < LP; ++i) s2 += X[c * CS + i] * X[c * CS + i];
                nrm[c] = s2;
            }
        if (tid == 0) {
            flags[0] = 0;
            flags[1] = 0;
        }
        __syncthreads();
        if (sweeps == 0) {
            C f = C(0);
            for (int c = 0; c < LP; ++c) f += nrm[c];
            negl = f * (C)((double)l * l * BEps<C>::eps * BEps<C>::eps);
        }
        for (int round = 0; round < N - 1; ++round) {
            if (active) {
                int p, q;
                brr_pair(round, pi, N, p, q);
                C xp[CH], xq[CH], jp[CH], jq[CH];
                const int i0 = sub * CH;
#pragma unroll
                for (int t = 0; t < CH; ++t) {
                    xp[t] = X[p * CS + i0 + t];
                    xq[t] = X[q * CS + i0 + t];
                    jp[t] = J[p * CS + i0 + t];
                    jq[t] = J[q * CS + i0 + t];
                }
                C a, b;
                if (round == 0 && sweeps > 0) {  // exact norms once per sweep; the rounds update them
                    C a0 = C(0), b0 = C(0);
#pragma unroll
                    for (int t = 0; t < CH; ++t) {
                        a0 += xp[t] * xp[t];
                        b0 += xq[t] * xq[t];
                    }
                    a = sum16(a0);
                    b = sum16(b0);
                    if (sub == 0) {
                        nrm[p] = a;
                        nrm[q] = b;
                    }
                } else {
                    a = nrm[p];
                    b = nrm[q];
                }
                C g0 = C(0);
#pragma unroll
                for (int t = 0; t < CH; ++t) g0 += xp[t] * xq[t];
                const C g = sum16(g0);
                const C gg = g * g, ab = a * b;
                if (g != C(0) && gg > tol2 * ab && a > negl && b > negl) {
                    const C d = b - a, g2 = C(2) * g;
                    const C hyp2 = d * d + g2 * g2;
                    C tmag;
                    if (hyp2 > (C)BEps<C>::lo && hyp2 < (C)BEps<C>::hi) {
                        const C hyp = hyp2 * brsqrt(hyp2);
                        tmag = fabs(g2) * brcp(fabs(d) + hyp);
                    } else {
                        const C sc = fmax(fabs(d), fabs(g2));
                        const C ds = fabs(d) / sc, gs = fabs(g2) / sc;
                        tmag = gs / (ds + sqrt(ds * ds + gs * gs));
                    }
                    const C t = ((d >= C(0)) == (g >= C(0))) ? tmag : -tmag;
                    const C cs = brsqrt(C(1) + t * t), sn = cs * t;
#pragma unroll
                    for (int u = 0; u < CH; ++u) {
                        X[p * CS + i0 + u] = cs * xp[u] - sn * xq[u];
                        X[q * CS + i0 + u] = sn * xp[u] + cs * xq[u];
                        J[p * CS + i0 + u] = cs * jp[u] - sn * jq[u];
                        J[q * CS + i0 + u] = sn * jp[u] + cs * jq[u];
                    }
                    if (sub == 0) {
                        nrm[p] = a - t * g;
                        nrm[q] = b + t * g;
                        flags[0] = 1;
                        if (gg > (C)BEps<C>::quad2 * ab) flags[1] = 1;
                    }
                }
            }
            __syncthreads();
        }
        if (flags[0] == 0 || flags[1] == 0) {
            ++sweeps;
            break;
        }
        __syncthreads();
    }
    for (int c = tid; c < LP; c += nt) {
        double s2 = 0.0;
        if (c < l)
            for (int i = 0; i < LP; ++i) s2 += (double)X[c * CS + i] * (double)X[c * CS + i];
        const double sv = sqrt(s2);
        sig[c] = (isfinite(sv) && s2 > (double)negl) ? sv : 0.0;
    }
    __syncthreads();
    for (int c = tid; c < LP; c += nt) {
        int rk = c;  // padding columns keep their own index
        if (c < l) {
            rk = 0;
            const double sc = sig[c];
            for (int d = 0; d < l; ++d) rk += (sig[d] > sc) || (sig[d] == sc && d < c);
        }
        rank[c] = rk;
    }
    __syncthreads();
    return sweeps;
}

// U_w in Ud (column k contiguous, fp64): the normalised rotated columns in descending order, the
// columns of zero singular values completed to an orthonormal basis as jacobi.hip does.
template <typename C, int LP>
__device__ __forceinline__ void build_uw(char* sm, int l) {
    typedef BShape<C, LP> SH;
    constexpr int CS = SH::CS;
    const C* X = reinterpret_cast<const C*>(sm + SH::oX);
    double* Ud = reinterpret_cast<double*>(sm + SH::oUd);
    const double* sig = reinterpret_cast<const double*>(sm + SH::oSig);
    double* v = reinterpret_cast<double*>(sm + SH::oV);
    const int* rank = reinterpret_cast<const int*>(sm + SH::oRank);
    int* flags = reinterpret_cast<int*>(sm + SH::oFlags);
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < LP * LP; e += nt) Ud[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < l * l; e += nt) {
        const int c = e / l, i = e % l;
        if (sig[c] > 0.0) Ud[rank[c] * LP + i] = (double)X[c * CS + i] / sig[c];
    }
    __syncthreads();
    int nz = 0;
    for (int c = 0; c < l; ++c) nz += (sig[c] > 0.0);
    for (int k = nz; k < l; ++k) {
        for (int i = tid; i < LP; i += nt) {
            double cov = 0.0;
            for (int j = 0; j < k; ++j) cov += Ud[j * LP + i] * Ud[j * LP + i];
            v[i] = (i < l) ? cov : 1e300;
        }
        __syncthreads();
        if (tid == 0) {
            int best = 0;
            for (int i = 1; i < l; ++i)
                if (v[i] < v[best]) best = i;
            flags[2] = best;
        }
        __syncthreads();
        const int cand = flags[2];
        for (int i = tid; i < LP; i += nt) Ud[k * LP + i] = (i == cand) ? 1.0 : 0.0;
        __syncthreads();
        for (int pass = 0; pass < 2; ++pass) {
            for (int j = tid; j < k; j += nt) {
                double d = 0.0;
                for (int i = 0; i < l; ++i) d += Ud[j * LP + i] * Ud[k * LP + i];
                v[j] = d;
            }
            __syncthreads();
            for (int i = tid; i < l; i += nt) {
                double x = Ud[k * LP + i];
                for (int j = 0; j < k; ++j) x -= v[j] * Ud[j * LP + i];
                Ud[k * LP + i] = x;
            }
            __syncthreads();
        }
        if (tid == 0) {
            double nv = 0.0;
            for (int i = 0; i < l; ++i) nv += Ud[k * LP + i] * Ud[k * LP + i];
            v[0] = 1.0 / sqrt(nv);
        }
        __syncthreads();
        const double sc = v[0];
        for (int i = tid; i < l; i += nt) Ud[k * LP + i] *= sc;
        __syncthreads();
    }
}

// ---- the compress tail: C = U_k diag(S_k) V_k^T and its error, from what is still in LDS ---------
//
// P (rows x l, column-major ld rows) becomes, in place, the rows x k factor
//   F[i, r] = scale(r) * sum_t P[i, t] W[t, src(r)],   src(r) = inv ? inv[r] : r,
//   scale(r) = sig ? sig[src(r)] : 1.
// A row of F depends on the same row of P alone, so a round takes whole rows: every thread of the
// round reads its row into 8 accumulators, one barrier, then the row is overwritten.  Rounds touch
// disjoint rows and need no barrier between them.  W has LP >= 8 ceil(k / 8) columns and inv as many
// entries, so the columns past k of the last chunk are summed unclamped and dropped.  tid: the thread
// index through a value the compiler cannot see through, so that nothing derived from it is hoisted
// out of the kernel's loop over matrices into registers the projections need.
template <typename T, typename TW>
__device__ void scale_panel(int tid, T* P, int rows, int l, int k, const TW* W, int ldw, const int* inv,
                            const double* sig) {
    const int nch = (k + 7) / 8;
    const int R = blockDim.x / nch;  // rows of a round
    const int ch = tid / R, ri = tid % R;
    for (int r0 = 0; r0 < rows; r0 += R) {
        const int i = r0 + ri;
        const bool on = ch < nch && i < rows;
        double acc[8];
        int cc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            acc[c] = 0.0;
            cc[c] = (inv ? inv[ch * 8 + c] : ch * 8 + c) * ldw;
        }
        if (on)
            for (int t = 0; t < l; ++t) {
                const double pv = (double)P[i + t * rows];
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] = fma(pv, (double)W[t + cc[c]], acc[c]);
            }
        __syncthreads();
        if (on) {
#pragma unroll
            for (int c = 0; c < 8; ++c)
                if (ch * 8 + c < k) {
                    const int r = ch * 8 + c;
                    P[i + r * rows] = (T)(sig ? acc[c] * sig[inv ? inv[r] : r] : acc[c]);
                }
        }
    }
    __syncthreads();
}

// C (m x n, ldc; nullable) = asc Fm Fn^T with the projections' item shape (one row, 8 columns, the k sum
// in order, fp64 accumulators, scaled by asc = a_scale and rounded to T once: C of a scaled call is the
// unscaled C times a_scale to one rounding).  The item that owns C[i, j] also reads A[i, j] -- before it
// stores, so C may be A itself -- and adds (asc a)^2 and (asc a - c)^2 to its two fp64 sums.  Those
// are joined in a fixed order: per thread over its items, the 64-lane butterfly, the waves in index
// order.  part: 2 x waves fp64 words of scratch.
template <typename T>
__device__ void rebuild_tile(int tid, const T* Fm, int m, const T* Fn, int n, int k, const T* A, int64_t lda,
                             double asc, T* C, int64_t ldc, double* part, double* err2) {
#pragma clang fp contract(off)  // a - c is taken from C as stored, not from the unrounded product
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    const int nch = (n + 7) / 8;
    double sa = 0.0, se = 0.0;
    for (int it = tid; it < m * nch; it += blockDim.x) {
        const int i = it % m, j0 = (it / m) * 8;
        double acc[8];
        int cc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            acc[c] = 0.0;
            cc[c] = j0 + c < n ? j0 + c : n - 1;
        }
        for (int r = 0; r < k; ++r) {
            const double f = (double)Fm[i + r * m];
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fma(f, (double)Fn[cc[c] + r * n], acc[c]);
        }
        const T* ap = A + i + (int64_t)j0 * lda;  // one column at a time: the two sums are a chain anyway
        T* cp = C ? C + i + (int64_t)j0 * ldc : nullptr;
#pragma unroll
        for (int c = 0; c < 8; ++c)
            if (j0 + c < n) {
                const T cv = (T)(acc[c] * asc);
                const double av = (double)*ap * asc;
                const double d = av - (double)cv;
                sa = fma(av, av, sa);
                se = fma(d, d, se);
                if (cp) {
                    *cp = cv;
                    cp += ldc;
                }
                ap += lda;
            }
    }
    sa = warp_sum(sa);
    se = warp_sum(se);
    if (lane == 0) {
        part[2 * wave] = sa;
        part[2 * wave + 1] = se;
    }
    __syncthreads();
    if (tid == 0 && err2) {
        double ta = 0.0, te = 0.0;
        for (int w = 0; w < nw; ++w) {
            ta += part[2 * w];
            te += part[2 * w + 1];
        }
        err2[0] = ta;
        err2[1] = te;
    }
    __syncthreads();
}

// Waves per SIMD the register allocation must leave room for.  The instantiations below sit at exactly
// 128 VGPRs (four waves); the handful of values the exact scaling of W adds would otherwise tip them to
// 130 and three waves, which costs the fp32 tile shapes of tools/batched_bench.py 60 to 80 per cent.
template <typename T, int LP, bool COMP>
constexpr int batched_min_waves() {
    return (!COMP && (LP == 16 || (sizeof(T) == 4 && LP <= 48))) ? 4 : 1;
}

template <typename T, int LP, bool PLDS, bool COMP>
__global__ __launch_bounds__((BShape<T, LP>::NT)) __attribute__((amdgpu_waves_per_eu(batched_min_waves<T, LP, COMP>())))
void batched_rsvd_kernel(BatchedArgs a) {
    typedef BShape<T, LP> SH;
    constexpr int CS = SH::CS;
    extern __shared__ __attribute__((aligned(16))) char bsm[];
    T* X = reinterpret_cast<T*>(bsm + SH::oX);
    T* J = reinterpret_cast<T*>(bsm + SH::oJ);
    double* Ud = reinterpret_cast<double*>(bsm + SH::oUd);
    double* sig = reinterpret_cast<double*>(bsm + SH::oSig);
    double* scr = reinterpret_cast<double*>(bsm + SH::oV);
    double* tau = reinterpret_cast<double*>(bsm + SH::oTau);
    int* rank = reinterpret_cast<int*>(bsm + SH::oRank);
    int* flags = reinterpret_cast<int*>(bsm + SH::oFlags);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int m = a.m, n = a.n, l = a.l;
    T* Pm = PLDS ? reinterpret_cast<T*>(bsm + SH::bytes)
                 : reinterpret_cast<T*>(a.ws + (size_t)blockIdx.x * a.ws_slice);
    T* Pn = Pm + (size_t)m * l;

    for (int64_t b = blockIdx.x; b < a.batch; b += gridDim.x) {
        const int64_t i0 = b % a.count0, i1 = b / a.count0;
        const T* A = reinterpret_cast<const T*>(a.A) + i0 * a.a_stride0 + i1 * a.a_stride1;
        T* Ub = reinterpret_cast<T*>(a.U) + b * a.u_stride;
        T* Sb = reinterpret_cast<T*>(a.S) + b * a.s_stride;
        T* Vb = reinterpret_cast<T*>(a.V) + b * a.v_stride;
        if (tid == 0) {
            flags[kFlDeficient] = 0;
            flags[kFlNonFinite] = 0;
            flags[kFlWexp] = 0;
        }
        // Omega
        if (a.omega) {
            const T* om = reinterpret_cast<const T*>(a.omega) + b * a.omega_stride;
            for (int e = tid; e < n * l; e += nt) {
                const int j = e % n, c = e / n;
                Pn[e] = om[j + (int64_t)c * a.ldo];
            }
        } else {
            const uint64_t seed = a.seed + (uint64_t)b;
            for (int e = tid; e < n * l; e += nt) Pn[e] = (T)gauss_elem((uint64_t)e, seed);  // e = j + n c
        }
        __syncthreads();
        // range finder
        gemm_nn<T, T, T>(A, a.lda, m, n, Pn, n, l, Pm, m, nullptr, 1.0);
        __syncthreads();
        house_factor<T>(Pm, m, l, tau, scr, flags);
        house_form_q<T>(Pm, m, l, tau);
        for (int it = 0; it < a.q; ++it) {
            gemm_tn<T>(A, a.lda, m, n, Pm, m, l, Pn, n);
            __syncthreads();
            house_factor<T>(Pn, n, l, tau, scr, flags);
            house_form_q<T>(Pn, n, l, tau);
            gemm_nn<T, T, T>(A, a.lda, m, n, Pn, n, l, Pm, m, nullptr, 1.0);
            __syncthreads();
            house_factor<T>(Pm, m, l, tau, scr, flags);
            house_form_q<T>(Pm, m, l, tau);
        }
        // B^T = A^T Q = Q_B R; W = R^T goes to the Jacobi columns: X[c][i] = W[i][c] = R[c][i]
        gemm_tn<T>(A, a.lda, m, n, Pm, m, l, Pn, n);
        __syncthreads();
        house_factor<T>(Pn, n, l, tau, scr, flags);
        T wmax = T(0);
        for (int e = tid; e < LP * LP; e += nt) {
            const int c = e / LP, i = e % LP;
            T x = T(0);
            if (c < l && i < l && i >= c) {
                x = Pn[c + i * n];
                if (!isfinite(x)) flags[kFlNonFinite] = 1;  // Inf / NaN in A reach R whatever came before
                else wmax = fmax(wmax, fabs(x));
            }
            X[c * CS + i] = x;
            J[c * CS + i] = (c == i && c < l) ? T(1) : T(0);
        }
        if (wmax > T(0)) atomicMax(&flags[kFlWexp], frexp_exp(wmax) + 2048);
        __syncthreads();
        // W / 2^wexp (jacobi.hip: the rotation test compares fourth powers of the singular values, so
        // the sweeps run on entries of order 1 and S is scaled back below; the scaling is exact).
        // Every thread scales the entries it stored itself.
        // wexp is read back from LDS wherever it is needed (wexp_of), not kept in a register across
        // the Jacobi: two more live registers cost the fp32 kernels a wave of occupancy.
        {
            const int wraw = flags[kFlWexp] ? flags[kFlWexp] - 2048 : 0;
            if (tid == 0 && (wraw > BEps<T>::emax || wraw < -BEps<T>::emax)) flags[kFlNonFinite] = 1;
            const int wexp = wexp_of<T>(flags);
            if (wexp != 0) {
                const T wscale = (T)pow2(-wexp);
                int st = tid;  // (opaque, as ct below: no index of this loop is hoisted out of the loop over matrices)
                asm volatile("" : "+v"(st));
                for (int e = st; e < LP * LP; e += nt) X[(e / LP) * CS + e % LP] *= wscale;
            }
        }
        __syncthreads();
        house_form_q<T>(Pn, n, l, tau);
        const int sweeps = jacobi_lds<T, LP>(bsm, l);
        // V = Q_B V_w (column rank[c] from rotation column c), S, then U = Q U_w
        const bool factors = !COMP || a.U != nullptr;  // a compress call may keep them out of global memory
        if (factors) gemm_nn<T, T, T>(Pn, n, n, l, J, CS, l, Vb, a.ldv, rank, a.v_neg ? -1.0 : 1.0);
        for (int c = tid; c < l; c += nt) {
            const double sback = pow2(wexp_of<T>(flags));  // sig is that of W / 2^wexp
            const T sv = (T)(sig[c] * sback * a.s_scale);
            if (!isfinite(sv)) flags[kFlNonFinite] = 1;
            if (factors) Sb[rank[c]] = sv;
        }
        build_uw<T, LP>(bsm, l);
        if (factors) gemm_nn<T, double, T>(Pm, m, m, l, Ud, LP, l, Ub, a.ldu, nullptr, 1.0);
        __syncthreads();
        if (COMP) {
            // Pm <- U_k = Pm U_w[:, :k]; Pn <- Pn V_w[:, column of rank r] * sigma_r; then
            // C = a_scale Pm Pn^T (|a_scale| is S's, the sign V's) against a_scale A.  tau is free after
            // the last Q: it holds the inverse of rank[].
            int* inv = reinterpret_cast<int*>(tau);
            for (int c = tid; c < LP; c += nt) {
                inv[rank[c]] = c;  // padding columns keep their own index
                sig[c] *= pow2(wexp_of<T>(flags));  // the rebuild takes the singular values of W itself
            }
            __syncthreads();
            int ct = tid;
            asm volatile("" : "+v"(ct));
            const double asc = a.v_neg ? -a.s_scale : a.s_scale;
            scale_panel<T, double>(ct, Pm, m, l, a.k, Ud, LP, nullptr, nullptr);
            scale_panel<T, T>(ct, Pn, n, l, a.k, J, CS, inv, sig);
            T* Cb = a.C ? reinterpret_cast<T*>(a.C) + i0 * a.c_stride0 + i1 * a.c_stride1 : nullptr;
            rebuild_tile<T>(ct, Pm, m, Pn, n, a.k, A, a.lda, asc, Cb, a.ldc, scr,
                            a.err2 ? a.err2 + 2 * b : nullptr);
        }
        if (tid == 0) {
            const int nf = flags[kFlNonFinite];
            if (nf) atomicOr(a.nonfinite, 1);
            if (a.info) {
                a.info[2 * b] = sweeps;
                a.info[2 * b + 1] = (flags[kFlDeficient] ? 1 : 0) | (nf ? 2 : 0);
            }
        }
        __syncthreads();
    }
}

template <typename T, int LP, bool COMP>
hipError_t launch_tl(const BatchedArgs& a, bool plds, size_t lds, int grid, hipStream_t s) {
    typedef BShape<T, LP> SH;
    if (plds)
        hipLaunchKernelGGL((batched_rsvd_kernel<T, LP, true, COMP>), dim3(grid), dim3(SH::NT), lds, s, a);
    else
        hipLaunchKernelGGL((batched_rsvd_kernel<T, LP, false, COMP>), dim3(grid), dim3(SH::NT), lds, s, a);
    return hipGetLastError();
}

template <typename T, bool COMP>
hipError_t launch_t(const BatchedArgs& a, int LP, bool plds, size_t lds, int grid, hipStream_t s) {
    switch (LP) {
        case 16: return launch_tl<T, 16, COMP>(a, plds, lds, grid, s);
        case 32: return launch_tl<T, 32, COMP>(a, plds, lds, grid, s);
        case 48: return launch_tl<T, 48, COMP>(a, plds, lds, grid, s);
        case 64: return launch_tl<T, 64, COMP>(a, plds, lds, grid, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

size_t batched_small_bytes(int dtype, int LP) {
    const bool f64 = dtype == 0;
    switch (LP) {
        case 16: return f64 ? BShape<double, 16>::bytes : BShape<float, 16>::bytes;
        case 32: return f64 ? BShape<double, 32>::bytes : BShape<float, 32>::bytes;
        case 48: return f64 ? BShape<double, 48>::bytes : BShape<float, 48>::bytes;
        default: return f64 ? BShape<double, 64>::bytes : BShape<float, 64>::bytes;
    }
}

size_t batched_panel_bytes(int dtype, int m, int n, int l) {
    const size_t b = (size_t)(dtype == 0 ? 8 : 4) * ((size_t)m + n) * l;
    return (b + 255) & ~size_t(255);
}

hipError_t launch_batched_rsvd(const BatchedArgs& a, int dtype, int LP, bool panels_in_lds, size_t lds_bytes, int grid,
                               hipStream_t s) {
    if (dtype == 0) return launch_t<double, false>(a, LP, panels_in_lds, lds_bytes, grid, s);
    return launch_t<float, false>(a, LP, panels_in_lds, lds_bytes, grid, s);
}

hipError_t launch_batched_compress(const BatchedArgs& a, int dtype, int LP, bool panels_in_lds, size_t lds_bytes,
                                   int grid, hipStream_t s) {
    if (dtype == 0) return launch_t<double, true>(a, LP, panels_in_lds, lds_bytes, grid, s);
    return launch_t<float, true>(a, LP, panels_in_lds, lds_bytes, grid, s);
}

}  // namespace rsvd
