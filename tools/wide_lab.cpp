// wide_lab.cpp -- hipEvent timings of the wide-engine kernels on synthetic inputs (tuning aid).
// Build: make -C rsvd_kamaneh_raganato_terrana_amd/csrc widelab ; run on the GPU box:
//   tools/wide_lab [what]   what in {all, pg, gram, chol, jac, proj}
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <vector>

#include "../rsvd_kamaneh_raganato_terrana_amd/csrc/kernels.hpp"
#include "../rsvd_kamaneh_raganato_terrana_amd/csrc/wide.hpp"

using namespace rsvd;

#define CK(x)                                                                                    \
    do {                                                                                         \
        hipError_t e = (x);                                                                      \
        if (e != hipSuccess) {                                                                   \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e));     \
            exit(1);                                                                             \
        }                                                                                        \
    } while (0)

static hipStream_t S;

static double time_us(const std::function<void()>& f, int reps = 5) {
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    f();
    CK(hipStreamSynchronize(S));
    std::vector<float> t;
    for (int i = 0; i < reps; ++i) {
        CK(hipEventRecord(a, S));
        f();
        CK(hipEventRecord(b, S));
        CK(hipEventSynchronize(b));
        float ms;
        CK(hipEventElapsedTime(&ms, a, b));
        t.push_back(ms * 1e3f);
    }
    std::sort(t.begin(), t.end());
    CK(hipEventDestroy(a));
    CK(hipEventDestroy(b));
    return t[t.size() / 2];
}

template <typename T>
static T* dev_random(size_t n, float scale = 1.0f, unsigned seed = 1) {
    std::vector<T> h(n);
    std::mt19937 g(seed);
    std::normal_distribution<float> d(0.f, scale);
    for (auto& x : h) x = (T)d(g);
    T* p;
    CK(hipMalloc(&p, n * sizeof(T)));
    CK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
    return p;
}

static void bench_pg() {
    for (int LP : {128, 256, 512}) {
        const int64_t rows = LP == 128 ? (1 << 20) : (LP == 256 ? 65536 : 131072);
        float* In = dev_random<float>((size_t)rows * LP);
        float* Out;
        bf16_t *hi, *lo;
        CK(hipMalloc(&Out, (size_t)rows * LP * 4));
        CK(hipMalloc(&hi, (size_t)rows * LP * 2));
        CK(hipMalloc(&lo, (size_t)rows * LP * 2));
        float* M = dev_random<float>((size_t)LP * LP, 0.1f);
        const double gb = (double)rows * LP * 4 * 2 / 1e9;
        double t0 = time_us([&] { CK(launch_panel_gemm<float>(In, rows, LP, M, 1, Out, 0, 0, nullptr, nullptr, nullptr, S)); });
        double t1 = time_us([&] { CK(launch_panel_gemm<float>(In, rows, LP, M, 1, Out, 0, 0, hi, lo, nullptr, S)); });
        double t2 = time_us([&] { CK(launch_panel_gemm<float>(In, rows, LP, M, 0, Out, rows, LP, nullptr, nullptr, nullptr, S)); });
        double t3 = time_us([&] { CK(launch_split_bf16<float>(In, rows, LP, hi, lo, S)); });
        printf("panel_gemm rows=%ld LP=%d: upper %.1f us (%.0f GB/s)  +hi/lo %.1f us  general->colmajor %.1f us  split_bf16 %.1f us\n",
               (long)rows, LP, t0, gb / t0 * 1e6 / 1e3, t1, t2, t3);
        CK(hipFree(In)); CK(hipFree(Out)); CK(hipFree(hi)); CK(hipFree(lo)); CK(hipFree(M));
    }
}

static void bench_psplit() {  // the split panel product (panel_split_kernel), C3 / C4 / C5 m-side shapes
    for (int LP : {128, 256, 512}) {
        if (std::getenv("LAB_LP") && std::atoi(std::getenv("LAB_LP")) != LP) continue;
        const int64_t rows = LP == 128 ? (1 << 20) : (LP == 256 ? 65536 : 131072);
        float* In = dev_random<float>((size_t)rows * LP);
        float* Out;
        bf16_t *hi, *lo, *ms;
        CK(hipMalloc(&Out, (size_t)rows * LP * 4));
        CK(hipMalloc(&hi, (size_t)rows * LP * 2));
        CK(hipMalloc(&lo, (size_t)rows * LP * 2));
        CK(hipMalloc(&ms, (size_t)3 * LP * LP * 2));
        float* M = dev_random<float>((size_t)LP * LP, 0.1f);
        const double gb = (double)rows * LP * (4 + 4 + 2 + 2) / 1e9;
        double t = time_us([&] { CK(launch_panel_gemm<float>(In, rows, LP, M, 1, Out, 0, 0, hi, lo, nullptr, S, ms)); });
        printf("panel_split rows=%ld LP=%d: %.1f us (%.0f GB/s of In + Out + hi + lo)\n", (long)rows, LP, t, gb / t * 1e6);
        CK(hipFree(In)); CK(hipFree(Out)); CK(hipFree(hi)); CK(hipFree(lo)); CK(hipFree(ms)); CK(hipFree(M));
    }
}

static void bench_gram() {
    for (int LP : {128, 256, 512}) {
        const int64_t rows = LP == 128 ? (1 << 20) : (LP == 256 ? 65536 : 131072);
        float* P = dev_random<float>((size_t)rows * LP);
        GramPlan gp = plan_gram_wide(rows, LP, 0);
        double* slabs;
        double* G;
        CK(hipMalloc(&slabs, (size_t)gp.blocks * gp.chunks * 1024 * 8));
        CK(hipMalloc(&G, (size_t)LP * LP * 8));
        double t = time_us([&] { CK(launch_gram_wide<float>(P, nullptr, rows, LP, gp, slabs, G, nullptr, S)); });
        const double fl = 2.0 * rows * LP * LP * gp.blocks / ((LP / 32.0) * (LP / 32.0));
        printf("gram rows=%ld LP=%d blocks=%d chunks=%d: %.1f us  (%.1f TF/s fp64, %.0f GB/s)\n", (long)rows, LP, gp.blocks,
               gp.chunks, t, fl / t / 1e6, rows * LP * 4.0 / t / 1e3);
        {  // symmetric path vs the cross (all-blocks) path on the same panel
            GramPlan gx = plan_gram_wide(rows, LP, 1);
            double *sx, *Gx;
            CK(hipMalloc(&sx, (size_t)gx.blocks * gx.chunks * 1024 * 8));
            CK(hipMalloc(&Gx, (size_t)LP * LP * 8));
            CK(launch_gram_wide<float>(P, P, rows, LP, gx, sx, Gx, nullptr, S));
            CK(hipStreamSynchronize(S));
            std::vector<double> a((size_t)LP * LP), b((size_t)LP * LP);
            CK(hipMemcpy(a.data(), G, a.size() * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(b.data(), Gx, b.size() * 8, hipMemcpyDeviceToHost));
            double md = 0, mx = 0;
            for (size_t i = 0; i < a.size(); ++i) { md = std::max(md, std::fabs(a[i] - b[i])); mx = std::max(mx, std::fabs(b[i])); }
            printf("  sym vs cross: max |diff| %.3e (max |G| %.3e) %s\n", md, mx, md <= 1e-12 * mx ? "OK" : "MISMATCH");
            CK(hipFree(sx)); CK(hipFree(Gx));
        }
        CK(hipFree(P)); CK(hipFree(slabs)); CK(hipFree(G));
    }
}

static void bench_gsplit() {  // the split Gram (bf16 MFMA) against the fp64 Gram of the same panel
    for (int LP : {128, 256, 512}) {
        if (std::getenv("LAB_LP") && std::atoi(std::getenv("LAB_LP")) != LP) continue;
        const int64_t rows = LP == 128 ? (1 << 20) : (LP == 256 ? 65536 : 131072);
        float* P = dev_random<float>((size_t)rows * LP);
        GramPlan gp = plan_gram_wide(rows, LP, 0);
        double *slabs, *G, *G64;
        CK(hipMalloc(&slabs, (size_t)gp.blocks * gp.chunks * 1024 * 8));
        CK(hipMalloc(&G, (size_t)LP * LP * 8));
        CK(hipMalloc(&G64, (size_t)LP * LP * 8));
        double t = time_us([&] { CK(launch_gram_split(P, rows, LP, gp, slabs, G, S)); });
        CK(launch_gram_wide<float>(P, nullptr, rows, LP, gp, slabs, G64, nullptr, S));
        CK(hipStreamSynchronize(S));
        std::vector<double> a((size_t)LP * LP), b((size_t)LP * LP);
        CK(hipMemcpy(a.data(), G, a.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), G64, b.size() * 8, hipMemcpyDeviceToHost));
        double md = 0;
        for (int i = 0; i < LP; ++i)
            for (int j = i; j < LP; ++j)
                md = std::max(md, std::fabs(a[(size_t)i * LP + j] - b[(size_t)i * LP + j]) /
                                      std::sqrt(b[(size_t)i * LP + i] * b[(size_t)j * LP + j]));
        const double fl = 6.0 * rows * LP * (LP + 16);  // six bf16 products over the upper tile triangle
        printf("gram_split rows=%ld LP=%d chunks=%d: %.1f us (%.0f TF/s bf16 issued, %.0f GB/s)  max|dG|/sqrt(GiiGjj) %.2e\n",
               (long)rows, LP, gp.chunks, t, fl / t / 1e6, rows * LP * 4.0 / t / 1e3, md);
        CK(hipFree(P)); CK(hipFree(slabs)); CK(hipFree(G)); CK(hipFree(G64));
    }
}

static void bench_gcross() {  // R = X^T Y by the split (LP = 256 / 512) against the fp64 cross Gram
  for (int LP : {256, 512}) {
    const int64_t rows = LP == 256 ? 65536 : 8192;
    float* X = dev_random<float>((size_t)rows * LP, 1.0f, 1);
    float* Y = dev_random<float>((size_t)rows * LP, 1.0f, 2);
    GramPlan gp = plan_gram_wide(rows, LP, 1);
    double *slabs, *G, *G64;
    CK(hipMalloc(&slabs, (size_t)gp.blocks * gp.chunks * 1024 * 8));
    CK(hipMalloc(&G, (size_t)LP * LP * 8));
    CK(hipMalloc(&G64, (size_t)LP * LP * 8));
    double t = time_us([&] { CK(launch_gram_split_cross(X, Y, rows, LP, gp, slabs, G, S)); });
    double t64 = time_us([&] { CK(launch_gram_wide<float>(X, Y, rows, LP, gp, slabs, G64, nullptr, S)); });
    CK(hipStreamSynchronize(S));
    std::vector<double> a((size_t)LP * LP), b((size_t)LP * LP);
    CK(hipMemcpy(a.data(), G, a.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(b.data(), G64, b.size() * 8, hipMemcpyDeviceToHost));
    double md = 0, mx = 0;
    for (size_t i = 0; i < a.size(); ++i) {
        md = std::max(md, std::fabs(a[i] - b[i]));
        mx = std::max(mx, std::fabs(b[i]));
    }
    printf("gram_split_cross rows=%ld LP=%d: %.1f us (fp64 cross Gram %.1f us)  max|dR| %.3e  max|R| %.3e  (|X_i||Y_j| = %.0f)\n",
           (long)rows, LP, t, t64, md, mx, (double)rows);
    CK(hipFree(X)); CK(hipFree(Y)); CK(hipFree(slabs)); CK(hipFree(G)); CK(hipFree(G64));
  }
}

static double* spd(int LP, int l) {  // G = X^T X + I with X random l x l
    std::vector<double> X((size_t)l * l), G((size_t)LP * LP, 0.0);
    std::mt19937 g(3);
    std::normal_distribution<double> d;
    for (auto& x : X) x = d(g);
    for (int i = 0; i < l; ++i)
        for (int j = 0; j < l; ++j) {
            double s = (i == j) ? 1.0 : 0.0;
            for (int k = 0; k < l; ++k) s += X[(size_t)k * l + i] * X[(size_t)k * l + j];
            G[(size_t)i * LP + j] = s;
        }
    double* p;
    CK(hipMalloc(&p, G.size() * 8));
    CK(hipMemcpy(p, G.data(), G.size() * 8, hipMemcpyHostToDevice));
    return p;
}

#ifdef RSVD_CHOL_PROF
namespace rsvd { void chol_prof_dump(int LP, int variant); void chol_diag_bench(); }
#endif
static void bench_chol() {
#ifdef RSVD_CHOL_PROF
    rsvd::chol_diag_bench();
#endif
    for (int LP : {64, 128, 256, 512}) {
        double* G = spd(LP, LP);
        double *R, *Ri, *W;
        float* R32;
        int *cf, *fl;
        CK(hipMalloc(&R, (size_t)LP * LP * 8));
        CK(hipMalloc(&Ri, (size_t)LP * LP * 8));
        CK(hipMalloc(&W, (size_t)LP * LP * 8));
        CK(hipMalloc(&R32, (size_t)LP * LP * 4));
        CK(hipMalloc(&cf, LP * 4));
        CK(hipMalloc(&fl, 4));
        CK(hipMemset(fl, 0, 4));
        // A/B: the L2-resident chol_wide_kernel (variant 0) against the register-resident chol_reg_kernel (1)
        std::vector<double> hR0((size_t)LP * LP), hRi0((size_t)LP * LP);
        CholArgs a;
        a.G = G, a.l = LP, a.LP = LP, a.tol = 1e-13, a.R = R, a.Rinv = Ri, a.Rinv32 = R32;
        a.colflag = cf, a.flag = fl, a.work = W;
        a.lab_variant = 0;
        double t0 = time_us([&] { CK(launch_chol(a, S)); });
        CK(hipMemcpy(hR0.data(), R, hR0.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hRi0.data(), Ri, hRi0.size() * 8, hipMemcpyDeviceToHost));
        a.lab_variant = 2;
        double t = time_us([&] { CK(launch_chol(a, S)); });
        a.lab_variant = 1;
        // check R^T R = G and R Ri = I on the host
        std::vector<double> hR((size_t)LP * LP), hRi((size_t)LP * LP), hG((size_t)LP * LP);
        CK(hipMemcpy(hR.data(), R, hR.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hRi.data(), Ri, hRi.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(hG.data(), G, hG.size() * 8, hipMemcpyDeviceToHost));
        double e1 = 0, e2 = 0, ng = 0;
        for (int i = 0; i < LP; ++i)
            for (int j = 0; j < LP; ++j) {
                double s = 0, s2 = 0;
                for (int k = 0; k < LP; ++k) {
                    s += hR[(size_t)k * LP + i] * hR[(size_t)k * LP + j];
                    s2 += hR[(size_t)i * LP + k] * hRi[(size_t)k * LP + j];
                }
                e1 += (s - hG[(size_t)i * LP + j]) * (s - hG[(size_t)i * LP + j]);
                ng += hG[(size_t)i * LP + j] * hG[(size_t)i * LP + j];
                e2 += (s2 - (i == j)) * (s2 - (i == j));
            }
#ifdef RSVD_CHOL_PROF
        rsvd::chol_prof_dump(LP, LP == 512 ? 0 : 1);  // LP = 512 ran chol_wide_kernel
#endif
        const bool same = !memcmp(hR0.data(), hR.data(), hR.size() * 8) && !memcmp(hRi0.data(), hRi.data(), hRi.size() * 8);
        printf("chol LP=%d: wide %.1f us  reg %.1f us  bit-identical %d   |R^T R - G|/|G| = %.2e  |R Rinv - I| = %.2e\n", LP,
               t0, t, (int)same, sqrt(e1 / ng), sqrt(e2));
        for (int depth = 0; LP >= 256 && depth <= (LP == 512 ? 1 : 0); ++depth) {  // the two-level factor
            double* scr;
            CK(hipMalloc(&scr, chol_2level_scratch_doubles(LP, depth) * 8));
            a.depth = depth, a.scratch = scr;
            double t2 = time_us([&] { CK(launch_chol(a, S)); });
            CK(hipMemcpy(hR.data(), R, hR.size() * 8, hipMemcpyDeviceToHost));
            CK(hipMemcpy(hRi.data(), Ri, hRi.size() * 8, hipMemcpyDeviceToHost));
            double f1 = 0, f2 = 0;
            for (int i = 0; i < LP; ++i)
                for (int j = 0; j < LP; ++j) {
                    double s = 0, s2 = 0;
                    for (int k = 0; k < LP; ++k) {
                        s += hR[(size_t)k * LP + i] * hR[(size_t)k * LP + j];
                        s2 += hR[(size_t)i * LP + k] * hRi[(size_t)k * LP + j];
                    }
                    f1 += (s - hG[(size_t)i * LP + j]) * (s - hG[(size_t)i * LP + j]);
                    f2 += (s2 - (i == j)) * (s2 - (i == j));
                }
            printf("chol2 LP=%d depth %d: %.1f us   |R^T R - G|/|G| = %.2e  |R Rinv - I| = %.2e\n", LP, depth, t2,
                   sqrt(f1 / ng), sqrt(f2));
            CK(hipFree(scr));
        }
        CK(hipFree(G)); CK(hipFree(R)); CK(hipFree(Ri)); CK(hipFree(W)); CK(hipFree(R32)); CK(hipFree(cf)); CK(hipFree(fl));
    }
}

#ifdef RSVD_BJ_PROF
namespace rsvd { void bj_prof_dump(); }
#endif
// Householder-free modified Gram-Schmidt QR of an n x n column-major matrix (host, for inputs)
static void mgs(std::vector<double>& A, int n, std::vector<double>* Rout) {
    if (Rout) Rout->assign((size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < j; ++i) {
                double d = 0;
                for (int t = 0; t < n; ++t) d += A[(size_t)i * n + t] * A[(size_t)j * n + t];
                for (int t = 0; t < n; ++t) A[(size_t)j * n + t] -= d * A[(size_t)i * n + t];
                if (Rout) (*Rout)[(size_t)j * n + i] += d;  // R[i][j] column-major
            }
        double nn = 0;
        for (int t = 0; t < n; ++t) nn += A[(size_t)j * n + t] * A[(size_t)j * n + t];
        nn = sqrt(nn);
        for (int t = 0; t < n; ++t) A[(size_t)j * n + t] /= nn;
        if (Rout) (*Rout)[(size_t)j * n + j] = nn;
    }
}

// R (upper triangular, stored [c][i] = R(i, c) as the kernel reads it) of W^T where W has the
// singular values s: W = U diag(s) V^T with random orthogonal U, V, R = qr(W^T).R
static std::vector<double> make_R(int LP, const std::vector<double>& sv, unsigned seed) {
    std::mt19937 g(seed);
    std::normal_distribution<double> d;
    std::vector<double> U((size_t)LP * LP), V((size_t)LP * LP);
    for (auto& x : U) x = d(g);
    for (auto& x : V) x = d(g);
    mgs(U, LP, nullptr);
    mgs(V, LP, nullptr);
    std::vector<double> Wt((size_t)LP * LP, 0.0);  // W^T (column-major): W^T = V diag(s) U^T
    for (int j = 0; j < LP; ++j)        // column j of W^T = sum_k V[:,k] s_k U[j,k]
        for (int k = 0; k < LP; ++k) {
            const double f = sv[k] * U[(size_t)k * LP + j];
            for (int i = 0; i < LP; ++i) Wt[(size_t)j * LP + i] += V[(size_t)k * LP + i] * f;
        }
    std::vector<double> R;
    mgs(Wt, LP, &R);
    // kernel layout: hR[c * LP + i] = R(c, i)?  the kernel reads X[c][i] = W[i][c] = R[c][i] with R
    // row-major [c][i] = R(c, i) (upper: i >= c)
    std::vector<double> hR((size_t)LP * LP, 0.0);
    for (int c = 0; c < LP; ++c)
        for (int i = c; i < LP; ++i) hR[(size_t)c * LP + i] = R[(size_t)i * LP + c];
    return hR;
}

static void bench_jac() {
    for (int LP : {128, 256, 512}) {
        for (int kind = 0; kind < 2; ++kind) {
            std::vector<double> hR((size_t)LP * LP, 0.0);
            if (kind == 0) {
                // R: upper triangular with a 0.97^i graded diagonal + noise (like a QR-preconditioned B^T)
                std::mt19937 g(5);
                std::normal_distribution<double> d;
                for (int i = 0; i < LP; ++i)
                    for (int j = i; j < LP; ++j) hR[(size_t)i * LP + j] = (i == j ? 1.0 : 0.05 * d(g)) * pow(0.97, i);
            } else {
                // the C4 / C5 small SVD: 90 * 0.9^t down to a noise floor, then a tight cluster (0.146 .. 0.2)
                std::vector<double> sv(LP);
                std::mt19937 g(7);
                std::uniform_real_distribution<double> u(0.146, 0.2);
                for (int t = 0; t < LP; ++t) sv[t] = std::max(90.0 * pow(0.9, t), u(g));
                hR = make_R(LP, sv, 11);
            }
            double* R;
            CK(hipMalloc(&R, hR.size() * 8));
            CK(hipMemcpy(R, hR.data(), hR.size() * 8, hipMemcpyHostToDevice));
            double *X, *J, *Uw, *Vw, *Sd;
            unsigned* sync;
            int* info;
            CK(hipMalloc(&X, (size_t)2 * LP * LP * 8));
            CK(hipMalloc(&J, (size_t)2 * LP * LP * 8));
            CK(hipMalloc(&Uw, (size_t)LP * LP * 8));
            CK(hipMalloc(&Vw, (size_t)LP * LP * 8));
            CK(hipMalloc(&Sd, LP * 8));
            CK(hipMalloc(&sync, kBJSyncWords * 4));
            CK(hipMalloc(&info, 16 * 4));
            for (int pg = 0; pg < 6; ++pg) {  // prec 0: fp64 results, 1: fp32 results; G = 1, 2, 4 row groups
                const int prec = pg & 1, G = 1 << (pg >> 1);
                if (block_jacobi_groups(LP, LP, G) != G) continue;
                CK(hipMemset(info, 0, 64));
                const double q2 = prec ? 1e-8 : 1e-16, tc = prec ? kBJTolF32 : kBJTolF64;
                double t = time_us([&] { CK(launch_block_jacobi<double>(R, LP, LP, X, J, Uw, Vw, Sd, sync, info, S, q2, tc, G)); }, 3);
                int hinfo[4];
                CK(hipMemcpy(hinfo, info, 16, hipMemcpyDeviceToHost));
                std::vector<double> hS(LP);
                CK(hipMemcpy(hS.data(), Sd, LP * 8, hipMemcpyDeviceToHost));
#ifdef RSVD_BJ_PROF
                rsvd::bj_prof_dump();
#endif
                std::vector<double> hU((size_t)LP * LP), hV((size_t)LP * LP);
                CK(hipMemcpy(hU.data(), Uw, hU.size() * 8, hipMemcpyDeviceToHost));
                CK(hipMemcpy(hV.data(), Vw, hV.size() * 8, hipMemcpyDeviceToHost));
                double rec = 0, wn = 0, orth = 0, uorth = 0;  // W = R^T = Uw diag(S) Vw^T (row-major [row][col])
                for (int i = 0; i < LP; ++i)
                    for (int j = 0; j < LP; ++j) {
                        double a = 0, o = 0, uo = 0;
                        for (int k = 0; k < LP; ++k) {
                            a += hU[(size_t)i * LP + k] * hS[k] * hV[(size_t)j * LP + k];
                            o += hV[(size_t)k * LP + i] * hV[(size_t)k * LP + j];
                            uo += hU[(size_t)k * LP + i] * hU[(size_t)k * LP + j];
                        }
                        const double w = hR[(size_t)j * LP + i];
                        rec += (a - w) * (a - w);
                        wn += w * w;
                        orth += (o - (i == j)) * (o - (i == j));
                        uorth += (uo - (i == j)) * (uo - (i == j));
                    }
                printf("block_jacobi LP=%d G=%d %s %s: %.1f us  sweeps=%d timeout=%d  S[0]=%.6f S[last]=%.3e  |W-USV'|/|W|=%.2e  "
                       "|V'V-I|=%.2e |U'U-I|=%.2e\n",
                       LP, G, kind ? "c4-cluster" : "graded", prec ? "f32-out" : "f64-out", t, hinfo[0], hinfo[2], hS[0],
                       hS[LP - 1], sqrt(rec / wn), sqrt(orth), sqrt(uorth));
            }
            CK(hipFree(R)); CK(hipFree(X)); CK(hipFree(J)); CK(hipFree(Uw)); CK(hipFree(Vw)); CK(hipFree(Sd));
            CK(hipFree(sync)); CK(hipFree(info));
        }
    }
}

// random bf16 (N(0,1)-ish, 8 significant bits) or e4m3 bytes, filled on the device: real data
// holds the clock the bench sees (zero / constant operands run the MFMA loop at a higher clock)
__global__ void fill_random_kernel(uint16_t* p, size_t n16, int fp8) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t x = (uint32_t)(i * 2654435761u) ^ (uint32_t)(i >> 32) * 40503u;
        x ^= x >> 15; x *= 0x2c1b3c6dU; x ^= x >> 12; x *= 0x297a2d39U; x ^= x >> 15;
        if (fp8) {  // two e4m3 codes of magnitude < 16, random signs (no NaN codes)
            const uint32_t a = (x & 0x5F) | (x & 0x80), b = ((x >> 8) & 0x5F) | ((x >> 8) & 0x80);
            p[i] = (uint16_t)(a | (b << 8));
        } else {  // bf16 with exponent in [2^-4, 2^3], random mantissa and sign
            p[i] = (uint16_t)((x & 0x807F) | ((0x7B + ((x >> 7) & 7)) << 7));
        }
    }
}

// the plan runs the v3 kernels of bf16 A at LP 256 / 512 (wproj3_kernel, wproj3tn2_kernel)
static bool plan_is_v3(const WProjPlan& p) {
    return (p.kernel == WProjKernel::W3 && p.LP >= 256) || p.kernel == WProjKernel::W3Tn2;
}
// the v3 TN at LP = 256 with single-step A slots (wproj3_kernel) instead of wproj3tn2_kernel
static void plan_tn2_off(WProjPlan& p) {
    if (p.kernel == WProjKernel::W3Tn2) p.kernel = WProjKernel::W3;
}

static void bench_proj(bool c4only = false) {
    struct Case { int64_t m, n; int LP; int fp8; };
    for (Case c : {Case{1 << 20, 1024, 128, 0}, Case{65536, 65536, 256, 0}, Case{131072, 8192, 512, 1}}) {
        if (c4only && c.LP != 256) continue;
        const size_t esz = c.fp8 ? 1 : 2;
        void* A;
        CK(hipMalloc(&A, (size_t)c.m * c.n * esz));
        hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)c.m * c.n * esz / 2, c.fp8);
        CK(hipStreamSynchronize(S));
        const int64_t mx = std::max(c.m, c.n);
        bf16_t* Sh = dev_random<bf16_t>((size_t)mx * c.LP);
        bf16_t* Sl = dev_random<bf16_t>((size_t)mx * c.LP);
        float* Out;
        CK(hipMalloc(&Out, (size_t)mx * c.LP * 4));
        for (int v2 = c4only ? 1 : 0; v2 < 4; ++v2) {
            WProjPlan pnn = plan_wproj(c.m, c.n, c.LP, v2 > 0, true, c.fp8), ptn = plan_wproj(c.n, c.m, c.LP, v2 > 0, false, c.fp8);
            // row "v2": the plans off the v3 kernels (LP = 128, e4m3); bf16 at LP 256 / 512 has no v2 kernel
            const bool v3 = plan_is_v3(pnn) || plan_is_v3(ptn);
            if (v2 == 1 ? v3 : (v2 >= 2 && !v3)) continue;
            if (v2 == 3) plan_tn2_off(ptn);  // v3 TN with single-step A slots
            float* slabs;
            CK(hipMalloc(&slabs, (size_t)std::max<int64_t>(pnn.splits * c.m, ptn.splits * c.n) * c.LP * 4));
            const double bytes = (double)c.m * c.n * esz, fl = 2.0 * c.m * c.n * c.LP;
            double t1 = time_us([&] { CK(launch_wproj(A, c.m, c.m, c.n, Sh, nullptr, pnn, slabs, Out, S)); });
            double t2 = time_us([&] { CK(launch_wproj(A, c.m, c.m, c.n, Sh, Sl, pnn, slabs, Out, S)); });
            double t3 = time_us([&] { CK(launch_wproj(A, c.m, c.m, c.n, Sh, Sl, ptn, slabs, Out, S)); });
            printf("proj%s m=%ld n=%ld LP=%d fp8=%d: NN1 %.1f us (%.0f GB/s) NN2 %.1f us (%.0f GB/s, %.0f TF) TN2 %.1f us"
                   " (%.0f GB/s, %.0f TF) splits nn=%d tn=%d\n",
                   v2 == 3 ? "v3(tn1)" : (v2 == 2 ? "v3" : (v2 ? "v2" : "v1")), (long)c.m, (long)c.n, c.LP, c.fp8, t1, bytes / t1 / 1e3, t2, bytes / t2 / 1e3,
                   2 * fl / t2 / 1e6, t3, bytes / t3 / 1e3, 2 * fl / t3 / 1e6, pnn.splits, ptn.splits);
            CK(hipFree(slabs));
        }
        CK(hipFree(A)); CK(hipFree(Sh)); CK(hipFree(Sl)); CK(hipFree(Out));
    }
}

// C5 e4m3 TN / NN at LP = 512 with a power-of-two column stride (lda = m) against a padded one:
// the L2-set hypothesis for the TN A over-fetch (32-B column runs per k-step, 2^17-B stride)
static void bench_c5_stride() {
    const int64_t m = 131072, n = 8192;
    const int LP = 512;
    for (int64_t pad : {0, 256, 4096 + 256}) {
        const int64_t lda = m + pad;
        void* A;
        CK(hipMalloc(&A, (size_t)lda * n));
        hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)lda * n / 2, 1);
        bf16_t* Sh = dev_random<bf16_t>((size_t)m * LP);
        bf16_t* Sl = dev_random<bf16_t>((size_t)m * LP);
        float* Out;
        CK(hipMalloc(&Out, (size_t)m * LP * 4));
        WProjPlan pnn = plan_wproj(m, n, LP, true, true, true), ptn = plan_wproj(n, m, LP, true, false, true);
        float* slabs;
        CK(hipMalloc(&slabs, (size_t)std::max<int64_t>(pnn.splits * m, ptn.splits * n) * LP * 4));
        double t2 = time_us([&] { CK(launch_wproj(A, lda, m, n, Sh, Sl, pnn, slabs, Out, S)); });
        double t3 = time_us([&] { CK(launch_wproj(A, lda, m, n, Sh, Sl, ptn, slabs, Out, S)); });
        printf("C5 e4m3 LP=512 lda=m+%ld: NN2 %.1f us  TN2 %.1f us (%s / %s, splits nn=%d tn=%d)\n", (long)pad, t2, t3,
               wproj_kernel_name(pnn.kernel), wproj_kernel_name(ptn.kernel), pnn.splits, ptn.splits);
        CK(hipFree(slabs)); CK(hipFree(A)); CK(hipFree(Sh)); CK(hipFree(Sl)); CK(hipFree(Out));
    }
}

typedef __attribute__((address_space(3))) void* lds_vp;
__global__ void glds_probe(const uint32_t* src, uint32_t* out, int mode) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    uint32_t* sm = reinterpret_cast<uint32_t*>(smem);
    for (int i = threadIdx.x; i < 512; i += blockDim.x) sm[i] = 0xdeadbeef;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        const uint32_t* g = src + 4 * (63 - lane);
        if (mode == 0) __builtin_amdgcn_global_load_lds(g, (lds_vp)(smem + 256), 16, 0, 0);
        else {
            const uint32_t la = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(lds_vp)(smem + 256));
            asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(g), "s"(la) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 512; i += blockDim.x) out[i] = sm[i];
}

static void probe_glds() {
    std::vector<uint32_t> h(1024);
    for (int i = 0; i < 1024; ++i) h[i] = i;
    uint32_t *src, *out;
    CK(hipMalloc(&src, 4096));
    CK(hipMalloc(&out, 2048));
    CK(hipMemcpy(src, h.data(), 4096, hipMemcpyHostToDevice));
    for (int mode = 0; mode < 2; ++mode) {
        hipLaunchKernelGGL(glds_probe, dim3(1), dim3(256), 4096, S, src, out, mode);
        CK(hipStreamSynchronize(S));
        std::vector<uint32_t> o(512);
        CK(hipMemcpy(o.data(), out, 2048, hipMemcpyDeviceToHost));
        printf("glds mode %d: dwords 60..72:", mode);
        for (int i = 60; i < 72; ++i) printf(" %x", o[i]);
        printf("\n   first non-dead at");
        for (int i = 0; i < 512; ++i) if (o[i] != 0xdeadbeef) { printf(" %d (val %u)", i, o[i]); break; }
        int last = -1;
        for (int i = 0; i < 512; ++i) if (o[i] != 0xdeadbeef) last = i;
        printf(" last %d (val %u)\n", last, last >= 0 ? o[last] : 0);
    }
}

static uint16_t f2bf_h(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

static void check_proj() {  // v2 (LDS-DMA) against v1 on random bf16 / e4m3 data
    for (int fp8 = 0; fp8 < 2; ++fp8)
    for (int LP : {128, 256, 512}) {
        const int64_t m = 2048 + 72 - 8 * fp8, n = 1024 + 40 - 5 * fp8;  // ragged: K tails of 8 / 24 rows
        std::vector<uint16_t> hA((size_t)m * n), hS((size_t)std::max(m, n) * LP), hL(hS.size());
        std::mt19937 g(7);
        std::normal_distribution<float> d;
        if (fp8) {  // random e4m3 codes, no NaN (0x7f / 0xff)
            uint8_t* b = reinterpret_cast<uint8_t*>(hA.data());
            for (size_t i = 0; i < (size_t)m * n; ++i) {
                uint8_t c = (uint8_t)(g() & 0xff);
                if ((c & 0x7f) == 0x7f) c ^= 1;
                b[i] = c;
            }
        } else {
            for (auto& x : hA) x = f2bf_h(d(g));
        }
        for (size_t i = 0; i < hS.size(); ++i) {
            hS[i] = f2bf_h(d(g));
            hL[i] = f2bf_h(d(g) * 1e-3f);
        }
        bf16_t *A, *Sh, *Sl;
        const size_t srows = (size_t)((std::max(m, n) + 31) / 32 * 32);
        CK(hipMalloc(&A, hA.size() * 2));
        CK(hipMalloc(&Sh, srows * LP * 2));
        CK(hipMalloc(&Sl, srows * LP * 2));
        CK(hipMemset(Sh, 0, srows * LP * 2));
        CK(hipMemset(Sl, 0, srows * LP * 2));
        CK(hipMemcpy(A, hA.data(), hA.size() * 2, hipMemcpyHostToDevice));
        float *O1, *O2, *sl;
        const int64_t mx = std::max(m, n);
        CK(hipMalloc(&O1, mx * LP * 4));
        CK(hipMalloc(&O2, mx * LP * 4));
        CK(hipMalloc(&sl, (size_t)256 * mx * LP * 4));
        for (int nn = 0; nn < 2; ++nn) {
            const int64_t rows_s = nn ? n : m;  // S panel rows = K
            CK(hipMemset(Sh, 0, srows * LP * 2));
            CK(hipMemset(Sl, 0, srows * LP * 2));
            CK(hipMemcpy(Sh, hS.data(), rows_s * LP * 2, hipMemcpyHostToDevice));
            CK(hipMemcpy(Sl, hL.data(), rows_s * LP * 2, hipMemcpyHostToDevice));
            const int64_t ro = nn ? m : n, K = nn ? n : m;
            WProjPlan p1 = plan_wproj(ro, K, LP, false, nn, fp8), p2 = plan_wproj(ro, K, LP, true, nn, fp8);
            for (int m32 = 0; m32 < 2; ++m32) {
            if (m32 && !plan_is_v3(p2)) continue;
            if (m32) plan_tn2_off(p2);
            CK(launch_wproj(A, m, m, n, Sh, Sl, p1, sl, O1, S));
            CK(launch_wproj(A, m, m, n, Sh, Sl, p2, sl, O2, S));
            CK(hipStreamSynchronize(S));
            std::vector<float> a(ro * LP), b(ro * LP);
            CK(hipMemcpy(a.data(), O1, a.size() * 4, hipMemcpyDeviceToHost));
            CK(hipMemcpy(b.data(), O2, b.size() * 4, hipMemcpyDeviceToHost));
            double md = 0, mx2 = 0;
            for (size_t i = 0; i < a.size(); ++i) {
                md = std::max(md, (double)fabs(a[i] - b[i]));
                mx2 = std::max(mx2, (double)fabs(a[i]));
            }
            printf("check fp8=%d LP=%d %s %s: max|v1-v2| = %.3e (max|v1| = %.3e) v2 splits=%d chunk=%ld\n",
                   fp8, LP, nn ? "NN" : "TN", wproj_kernel_name(p2.kernel), md, mx2, p2.splits, (long)p2.chunk);
            }
        }
        CK(hipFree(A)); CK(hipFree(Sh)); CK(hipFree(Sl)); CK(hipFree(O1)); CK(hipFree(O2)); CK(hipFree(sl));
    }
}

// e4m3 x e4m3 sketch (launch_wproj_s8, fp8 MFMA) against the bf16 path on the same exact values
static void check_s8() {
    for (int LP : {256, 512}) {
        const int64_t m = 4096 + 16 * 3, n = 2048 + 32;
        const int64_t npad = (n + 31) / 32 * 32;
        std::vector<uint8_t> hA((size_t)m * n), hS8((size_t)npad * LP, 0);
        std::vector<uint16_t> hSb((size_t)npad * LP, 0);
        std::mt19937 g(11);
        auto code = [&]() {
            uint8_t c = (uint8_t)(g() & 0xff);
            if ((c & 0x7f) == 0x7f) c ^= 1;
            return c;
        };
        auto e4m3_to_f = [](uint8_t c) {
            const int sgn = c >> 7, e = (c >> 3) & 15, mm = c & 7;
            const float v = e ? std::ldexp(1.0f + mm / 8.0f, e - 7) : std::ldexp(mm / 8.0f, -6);
            return sgn ? -v : v;
        };
        for (auto& x : hA) x = code();
        for (int64_t i = 0; i < n; ++i)
            for (int c = 0; c < LP; ++c) {
                const uint8_t cd = code();
                hS8[(size_t)i * LP + c] = cd;
                const float f = e4m3_to_f(cd);
                uint32_t u;
                std::memcpy(&u, &f, 4);
                hSb[(size_t)i * LP + c] = (uint16_t)(u >> 16);  // exact: e4m3 has 4 significant bits
            }
        void* A;
        uint8_t* S8;
        bf16_t *Sb, *Sb2;
        float *O1, *O2, *sl;
        CK(hipMalloc(&A, hA.size()));
        CK(hipMalloc(&S8, hS8.size()));
        CK(hipMalloc(&Sb, hSb.size() * 2));
        CK(hipMalloc(&Sb2, hSb.size() * 2));
        CK(hipMalloc(&O1, m * LP * 4));
        CK(hipMalloc(&O2, m * LP * 4));
        CK(hipMalloc(&sl, (size_t)64 * m * LP * 4));
        CK(hipMemcpy(A, hA.data(), hA.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(S8, hS8.data(), hS8.size(), hipMemcpyHostToDevice));
        CK(hipMemcpy(Sb, hSb.data(), hSb.size() * 2, hipMemcpyHostToDevice));
        // the engine's own conversion bf16 -> e4m3 must reproduce the codes
        CK(launch_bf16_to_fp8(Sb, npad * LP, reinterpret_cast<fp8_t*>(Sb2), S));
        std::vector<uint8_t> back(hS8.size());
        CK(hipMemcpy(back.data(), Sb2, back.size(), hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (size_t i = 0; i < back.size(); ++i) {
            const bool z1 = (back[i] & 0x7f) == 0, z2 = (hS8[i] & 0x7f) == 0;  // +-0 may flip sign
            bad += !(back[i] == hS8[i] || (z1 && z2));
        }
        WProjPlan p = plan_wproj(m, n, LP, true, true, true);
        CK(launch_wproj(A, m, m, n, Sb, nullptr, p, sl, O1, S));
        CK(launch_wproj_s8(A, m, m, n, reinterpret_cast<const fp8_t*>(S8), p, sl, O2, S));
        CK(hipStreamSynchronize(S));
        std::vector<float> a(m * LP), b(m * LP);
        CK(hipMemcpy(a.data(), O1, a.size() * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(b.data(), O2, b.size() * 4, hipMemcpyDeviceToHost));
        double md = 0, mx = 0;
        for (size_t i = 0; i < a.size(); ++i) {
            md = std::max(md, (double)fabs(a[i] - b[i]));
            mx = std::max(mx, (double)fabs(a[i]));
        }
        const double bytes = (double)m * n;
        double t1 = time_us([&] { CK(launch_wproj(A, m, m, n, Sb, nullptr, p, sl, O1, S)); });
        double t2 = time_us([&] { CK(launch_wproj_s8(A, m, m, n, reinterpret_cast<const fp8_t*>(S8), p, sl, O2, S)); });
        printf("check_s8 LP=%d m=%ld n=%ld: max|bf16 path - fp8 path| = %.3e (max %.3e); bf16->e4m3 code mismatches %zu;"
               " bf16 path %.1f us, fp8 path %.1f us (%.0f GB/s)\n", LP, (long)m, (long)n, md, mx, bad, t1, t2,
               bytes / t2 / 1e3);
        CK(hipFree(A)); CK(hipFree(S8)); CK(hipFree(Sb)); CK(hipFree(Sb2)); CK(hipFree(O1)); CK(hipFree(O2));
        CK(hipFree(sl));
    }
    // C5 shape timing on random data
    const int64_t m = 131072, n = 8192;
    const int LP = 512;
    void* A;
    uint8_t* S8;
    bf16_t* Sb;
    float *O, *sl;
    CK(hipMalloc(&A, (size_t)m * n));
    hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)m * n / 2, 1);
    CK(hipMalloc(&S8, (size_t)n * LP));
    hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)S8, (size_t)n * LP / 2, 1);
    Sb = dev_random<bf16_t>((size_t)n * LP);
    CK(hipMalloc(&O, (size_t)m * LP * 4));
    CK(hipMalloc(&sl, (size_t)m * LP * 4));
    WProjPlan p = plan_wproj(m, n, LP, true, true, true);
    double t1 = time_us([&] { CK(launch_wproj(A, m, m, n, Sb, nullptr, p, sl, O, S)); });
    double t2 = time_us([&] { CK(launch_wproj_s8(A, m, m, n, reinterpret_cast<const fp8_t*>(S8), p, sl, O, S)); });
    const double fl = 2.0 * m * n * LP;
    printf("C5 sketch 131072x8192 e4m3, LP=512: bf16-MFMA path %.1f us (%.0f TF), fp8-MFMA path %.1f us (%.0f TF = %.3f "
           "of the 5033 TF fp8 dense peak), splits %d\n", t1, fl / t1 / 1e6, t2, fl / t2 / 1e6, fl / t2 / 1e6 / 5033.2,
           p.splits);
    CK(hipFree(A)); CK(hipFree(S8)); CK(hipFree(Sb)); CK(hipFree(O)); CK(hipFree(sl));
}

// LDS-DMA vs register-path load throughput per CU from an L2-resident (or HBM-sized) buffer:
// every wave moves `iters` x 1 KiB.  mode 0: global_load_lds_dwordx4 (8 in flight per wave);
// 1: global_load_dwordx4 to VGPRs + ds_write_b128; 2: global_load_dwordx4 only (summed).
// mixed stream as the C4 projection sees it: per 3 KiB, 1 KiB from a streaming (HBM) buffer and
// 2 KiB from a 2-MiB L2-resident one; DEPTH glds in flight per wave
template <int DEPTH>
__global__ __launch_bounds__(512) void dma_mix_kernel(const uint8_t* __restrict__ big, const uint8_t* __restrict__ hot,
                                                      int iters, float* out) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t base = ((size_t)blockIdx.x * 8 + w) * (size_t)iters * 1024;
    for (int i = 0; i < iters; ++i) {
        const uint8_t* g = (i % 3 == 0) ? big + base + (size_t)i * 1024 + lane * 16
                                        : hot + (((size_t)i * 1024 + (size_t)blockIdx.x * 8192) & ((2u << 20) - 1)) + lane * 16;
        char* l = smem + (w * 16 + (i & 15)) * 1024;
        __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
        __builtin_amdgcn_s_waitcnt((DEPTH & 0xF) | ((DEPTH >> 4) << 14) | (0x7 << 4) | (0xF << 8));
    }
    __builtin_amdgcn_s_waitcnt((0x7 << 4) | (0xF << 8));
    __syncthreads();
    out[blockIdx.x * 512 + threadIdx.x] = ((float*)smem)[threadIdx.x];
}

template <int MODE>
__global__ __launch_bounds__(512) void dma_bench_kernel(const uint8_t* __restrict__ src, size_t mask, int iters,
                                                        float* out) {
    extern __shared__ __attribute__((aligned(1024))) char smem[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    size_t base = ((size_t)blockIdx.x * 8 + w) * 1024 * 64;
    uint4 accu = make_uint4(0, 0, 0, 0);
    for (int i = 0; i < iters; ++i) {
        const uint8_t* g = src + ((base + (size_t)i * 1024) & mask) + lane * 16;
        char* l = smem + (w * 8 + (i & 7)) * 1024;
        if constexpr (MODE == 0) {
            __builtin_amdgcn_global_load_lds(g, (__attribute__((address_space(3))) void*)l, 16, 0, 0);
            if ((i & 7) == 7) __builtin_amdgcn_s_waitcnt((0 & 0xF) | (0x7 << 4) | (0xF << 8));
        } else if constexpr (MODE == 1) {
            const uint4 v = *reinterpret_cast<const uint4*>(g);
            *reinterpret_cast<uint4*>(l + lane * 16) = v;
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(g);
            accu.x += v.x; accu.y ^= v.y; accu.z += v.z; accu.w ^= v.w;
        }
    }
    __syncthreads();
    if (MODE == 2) out[blockIdx.x * 512 + threadIdx.x] = (float)(accu.x + accu.y + accu.z + accu.w);
    else out[blockIdx.x * 512 + threadIdx.x] = ((float*)smem)[threadIdx.x];
}

static void dma_bench() {
    uint8_t* src;
    const size_t big = (size_t)8 << 30;
    CK(hipMalloc(&src, big));
    CK(hipMemset(src, 1, big));
    float* out;
    CK(hipMalloc(&out, 256 * 512 * 4 * 4));
    for (size_t foot : {(size_t)2 << 20, (size_t)8 << 30}) {
        const int iters = 4096;
        const double bytes = 256.0 * 8 * iters * 1024;
        double t0 = time_us([&] { hipLaunchKernelGGL(dma_bench_kernel<0>, dim3(256), dim3(512), 65536, S, src, foot - 1, iters, out); });
        double t1 = time_us([&] { hipLaunchKernelGGL(dma_bench_kernel<1>, dim3(256), dim3(512), 65536, S, src, foot - 1, iters, out); });
        double t2 = time_us([&] { hipLaunchKernelGGL(dma_bench_kernel<2>, dim3(256), dim3(512), 65536, S, src, foot - 1, iters, out); });
        printf("dma footprint %zu MiB: glds %.1f us (%.0f GB/s = %.1f B/clk/CU @2.1GHz)  load+ds_write %.1f us (%.0f GB/s)  load only %.1f us (%.0f GB/s)\n",
               foot >> 20, t0, bytes / t0 / 1e3, bytes / t0 / 1e3 / 256 / 2.1, t1, bytes / t1 / 1e3, t2, bytes / t2 / 1e3);
    }
    {
        const int iters = 3 * 1024;
        const double bytes = 256.0 * 8 * iters * 1024;
        auto run = [&](auto kern) {
            return time_us([&] { hipLaunchKernelGGL(kern, dim3(256), dim3(512), 131072, S, src, src + ((size_t)7 << 30), iters, out); });
        };
        double t4 = run(dma_mix_kernel<4>), t8 = run(dma_mix_kernel<8>), t12 = run(dma_mix_kernel<12>), t15 = run(dma_mix_kernel<15>);
        printf("dma mix (1/3 HBM stream, 2/3 L2): depth 4 %.0f GB/s, 8 %.0f GB/s, 12 %.0f GB/s, 15 %.0f GB/s (B/clk/CU @2.1GHz: %.1f %.1f %.1f %.1f)\n",
               bytes / t4 / 1e3, bytes / t8 / 1e3, bytes / t12 / 1e3, bytes / t15 / 1e3, bytes / t4 / 1e3 / 537.6,
               bytes / t8 / 1e3 / 537.6, bytes / t12 / 1e3 / 537.6, bytes / t15 / 1e3 / 537.6);
    }
    CK(hipFree(src));
    CK(hipFree(out));
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::string what = argc > 1 ? argv[1] : "all";
    CK(hipStreamCreate(&S));
    if (what == "all" || what == "pg") bench_pg();
    if (what == "all" || what == "gram") bench_gram();
    if (what == "all" || what == "chol") bench_chol();
    if (what == "gsplit") bench_gsplit();
    if (what == "gcross") bench_gcross();
    if (what == "psplit") bench_psplit();
    if (what == "all" || what == "jac") bench_jac();
    if (what == "all" || what == "proj") bench_proj();
    if (what == "proj4") bench_proj(true);
    if (what == "c5stride") bench_c5_stride();
    if (what == "kn") {  // v3 knob sweep at C4: bit 0 non-temporal A, bit 1 s_setprio on waves 4-7
        const int64_t m = 65536, n = 65536;
        const int LP = 256;
        void* A;
        CK(hipMalloc(&A, (size_t)m * n * 2));
        hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)m * n, 0);
        bf16_t* Sh = dev_random<bf16_t>((size_t)m * LP);
        bf16_t* Sl = dev_random<bf16_t>((size_t)m * LP);
        float* Out;
        CK(hipMalloc(&Out, (size_t)m * LP * 4));
        for (int rep = 0; rep < 2; ++rep)
            for (int kn = 0; kn < 4; ++kn) {
                WProjPlan pn = plan_wproj(m, n, LP, true), pt = plan_wproj(n, m, LP, true, false, false);
                pn.kn = pt.kn = kn;
                double t0 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, nullptr, pn, nullptr, Out, S)); });
                double t1 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, Sl, pn, nullptr, Out, S)); });
                double t2 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, Sl, pt, nullptr, Out, S)); });
                printf("rep %d kn %d: NN1 %.1f us  NN2 %.1f us  TN2 %.1f us\n", rep, kn, t0, t1, t2);
            }
    }
    if (what == "abl") {  // v3 ablations at C4 (timing only; results meaningless)
        const int64_t m = 65536, n = 65536;
        const int LP = 256;
        void* A;
        CK(hipMalloc(&A, (size_t)m * n * 2));
        hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)m * n, 0);
        bf16_t* Sh = dev_random<bf16_t>((size_t)m * LP);
        bf16_t* Sl = dev_random<bf16_t>((size_t)m * LP);
        float* Out;
        CK(hipMalloc(&Out, (size_t)m * LP * 4));
        const double fl = 4.0 * m * n * LP;
        for (int ab = 0; ab < 8; ++ab) {
            WProjPlan pn = plan_wproj(m, n, LP, true), pt = plan_wproj(n, m, LP, true, false, false);
            pn.abl = pt.abl = ab;
            double t1 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, Sl, pn, nullptr, Out, S)); });
            double t2 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, Sl, pt, nullptr, Out, S)); });
            printf("abl %d (%s%s%s): NN2 %.1f us (%.0f TF)  TN2 %.1f us (%.0f TF)\n", ab, ab & 1 ? "nobar " : "",
                   ab & 2 ? "nodma " : "", ab & 4 ? "nolds" : "", t1, fl / t1 / 1e6, t2, fl / t2 / 1e6);
        }
    }
    if (what == "areg") {  // v3 with A staged through registers (abl 16) against LDS-DMA A (the engine)
        for (int cs = 0; cs < 2; ++cs) {
            const int64_t m = cs ? 65536 : 4160, n = cs ? 65536 : 3000;  // case 0: ragged K, bit-identity
            const int LP = 256;
            void* A;
            CK(hipMalloc(&A, (size_t)m * n * 2));
            hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)m * n, 0);
            bf16_t* Sh = dev_random<bf16_t>((size_t)(m > n ? m : n) * LP);
            bf16_t* Sl = dev_random<bf16_t>((size_t)(m > n ? m : n) * LP);
            float *O0, *O1;
            CK(hipMalloc(&O0, (size_t)(m > n ? m : n) * LP * 4));
            CK(hipMalloc(&O1, (size_t)(m > n ? m : n) * LP * 4));
            const double fl = 4.0 * m * n * LP;
            for (int nn = 1; nn >= 0; --nn) {
                WProjPlan p0 = nn ? plan_wproj(m, n, LP, true) : plan_wproj(n, m, LP, true, false, false);
                WProjPlan p1 = p0;  // p0: the engine's plan (LDS-DMA A)
                p1.abl = 16;        // the same kernel with register-staged A
                const int64_t ro = nn ? m : n;
                float* slabs = nullptr;  // K-split partial products (p.splits > 1 writes them)
                CK(hipMalloc(&slabs, (size_t)p0.splits * ro * LP * 4));
                printf("case %ldx%ld nn %d splits %d ...\n", (long)m, (long)n, nn, p0.splits);
                double t0 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, Sl, p0, slabs, O0, S)); });
                printf("  dma-A %.1f us\n", t0);
                double t1 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, Sl, p1, slabs, O1, S)); });
                CK(hipFree(slabs));
                std::vector<float> h0((size_t)ro * LP), h1((size_t)ro * LP);
                CK(hipMemcpy(h0.data(), O0, h0.size() * 4, hipMemcpyDeviceToHost));
                CK(hipMemcpy(h1.data(), O1, h1.size() * 4, hipMemcpyDeviceToHost));
                const bool same = !memcmp(h0.data(), h1.data(), h0.size() * 4);
                printf("areg %ldx%ld %s: dma-A %.1f us (%.0f TF)  reg-A %.1f us (%.0f TF)  bit-identical %d\n", (long)m,
                       (long)n, nn ? "NN2" : (p0.kernel == WProjKernel::W3Tn2 ? "TN2(v3 tn2)" : "TN2(v3)"), t0, fl / t0 / 1e6, t1, fl / t1 / 1e6, (int)same);
            }
            CK(hipFree(A)); CK(hipFree(Sh)); CK(hipFree(Sl)); CK(hipFree(O0)); CK(hipFree(O1));
        }
    }
    if (what == "tn128") {  // LP = 128 TN: v2 double-step stages (W2Ds) against the separate rings
        for (int cs = 0; cs < 2; ++cs) {
            const int64_t m = cs ? (1 << 20) : 4160, n = cs ? 1024 : 1000;  // case 0: ragged rows, K chunks
            const int LP = 128;
            void* A;
            CK(hipMalloc(&A, (size_t)m * n * 2));
            hipLaunchKernelGGL(fill_random_kernel, dim3(4096), dim3(256), 0, S, (uint16_t*)A, (size_t)m * n, 0);
            bf16_t* Sh = dev_random<bf16_t>((size_t)m * LP);
            bf16_t* Sl = dev_random<bf16_t>((size_t)m * LP);
            float *O0, *O1;
            CK(hipMalloc(&O0, (size_t)n * LP * 4));
            CK(hipMalloc(&O1, (size_t)n * LP * 4));
            WProjPlan p0 = plan_wproj(n, m, LP, true, false, false), p1 = p0, p2 = p0;
            // (m a multiple of 64 in both cases: the planner's double-step choice, whatever RSVD_TN128 says)
            p0.kernel = WProjKernel::W2Ds;
            p1.kernel = p2.kernel = WProjKernel::W3Tn128;
            p2.rings33 = true;
            float* slabs;
            CK(hipMalloc(&slabs, (size_t)p0.splits * n * LP * 4));
            const double bytes = (double)m * n * 2;
            for (int sp = 1; sp >= 0; --sp) {
                const bf16_t* lo = sp ? Sl : nullptr;
                for (int rep = 0; rep < 2; ++rep) {
                    double t0 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, lo, p0, slabs, O0, S)); });
                    std::vector<float> h0((size_t)n * LP), h1((size_t)n * LP);
                    CK(hipMemcpy(h0.data(), O0, h0.size() * 4, hipMemcpyDeviceToHost));
                    double t1 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, lo, p1, slabs, O1, S)); });
                    CK(hipMemcpy(h1.data(), O1, h1.size() * 4, hipMemcpyDeviceToHost));
                    const bool same1 = !memcmp(h0.data(), h1.data(), h0.size() * 4);
                    CK(hipMemset(O1, 0, h1.size() * 4));
                    double t2 = time_us([&] { CK(launch_wproj(A, m, m, n, Sh, lo, p2, slabs, O1, S)); });
                    CK(hipMemcpy(h1.data(), O1, h1.size() * 4, hipMemcpyDeviceToHost));
                    const bool same2 = !memcmp(h0.data(), h1.data(), h0.size() * 4);
                    printf("tn128 %ldx%ld TN%d splits %d: v2ds %.1f us (%.0f GB/s)  rings 4/2 %.1f us (%.0f GB/s) same %d"
                           "  rings 3/3 %.1f us (%.0f GB/s) same %d\n",
                           (long)m, (long)n, sp ? 2 : 1, p0.splits, t0, bytes / t0 / 1e3, t1, bytes / t1 / 1e3, (int)same1,
                           t2, bytes / t2 / 1e3, (int)same2);
                }
            }
            CK(hipFree(slabs)); CK(hipFree(A)); CK(hipFree(Sh)); CK(hipFree(Sl)); CK(hipFree(O0)); CK(hipFree(O1));
        }
    }
    if (what == "all" || what == "check") check_proj();
    if (what == "probe") probe_glds();
    if (what == "s8") check_s8();
    if (what == "dma") dma_bench();
    CK(hipStreamDestroy(S));
    return 0;
}
