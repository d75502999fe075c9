// compress_test.cpp -- rsvd::compress (include/rsvd.hpp over rsvd_compress_host_f64) on a minimal
// column-major matrix type.  A[i, j] = 100 i + j + 1 (100 x 100) has rank 2, so its rank-2 rebuild from an
// rSVD of width 10 is A itself: ||A - C||_F <= 1e-9 ||A||_F for the whole matrix and for every tile
// of a 2 x 2 grid of 50 x 50 tiles (a block of a rank-2 matrix has rank <= 2), and the error words that
// come back agree with the norms recomputed here.
// Built by tests/test_cpp_compress.py with the flags of tests/cpp/Makefile; exit 0 = pass.
#include <cmath>
#include <cstdio>
#include <vector>

#include "rsvd.hpp"

struct HostMat {  // column-major, ld == rows
    long r = 0, c = 0;
    std::vector<double> v;
    long rows() const { return r; }
    long cols() const { return c; }
    double* data() { return v.data(); }
    const double* data() const { return v.data(); }
    void resize(long rr, long cc) { r = rr; c = cc; v.assign((size_t)rr * cc, 0.0); }
    double& operator()(long i, long j) { return v[(size_t)i + (size_t)j * r]; }
    double operator()(long i, long j) const { return v[(size_t)i + (size_t)j * r]; }
};

static int fails = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAIL: " __VA_ARGS__); \
            std::printf("\n");                 \
            ++fails;                           \
        }                                      \
    } while (0)

// ||A||_F^2 and ||A - C||_F^2 over rows [i0, i0 + tm) x columns [j0, j0 + tn)
static void norms(const HostMat& A, const HostMat& C, long i0, long j0, long tm, long tn, double* a2, double* e2) {
    *a2 = *e2 = 0.0;
    for (long j = j0; j < j0 + tn; ++j)
        for (long i = i0; i < i0 + tm; ++i) {
            const double a = A(i, j), d = a - C(i, j);
            *a2 += a * a;
            *e2 += d * d;
        }
}

int main() {
    const int n = 100, l = 10, k = 2;
    HostMat A, C;
    A.resize(n, n);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) A(i, j) = 100.0 * i + j + 1.0;

    std::vector<double> err;
    rsvd::compress(A, C, l, k, 0, 0, 2, &err);
    double a2, e2;
    norms(A, C, 0, 0, n, n, &a2, &e2);
    std::printf("whole matrix: ||A - C|| / ||A|| = %.3e (err2 %.6e %.3e)\n", std::sqrt(e2 / a2), err[0], err[1]);
    CHECK(C.rows() == n && C.cols() == n && err.size() == 2, "shapes");
    CHECK(std::sqrt(e2) <= 1e-9 * std::sqrt(a2), "rank-2 rebuild of a rank-2 matrix: %.3e", std::sqrt(e2 / a2));
    CHECK(std::fabs(err[0] - a2) <= 1e-10 * a2, "err2[0] %.17g against %.17g", err[0], a2);
    CHECK(err[1] <= 1e-18 * a2 && std::fabs(err[1] - e2) <= 1e-10 * e2 + 1e-30 * a2, "err2[1] %.3e against %.3e", err[1], e2);

    HostMat T;
    rsvd::compress(A, T, l, k, 50, 50, 2, &err);
    CHECK(err.size() == 8, "2 x 2 tiles give 8 error words");
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) {
            norms(A, T, 50 * i, 50 * j, 50, 50, &a2, &e2);
            const double* w = &err[2 * (i + 2 * j)];
            std::printf("tile (%d, %d): ||A - C|| / ||A|| = %.3e (err2 %.6e %.3e)\n", i, j, std::sqrt(e2 / a2), w[0], w[1]);
            CHECK(std::sqrt(e2) <= 1e-9 * std::sqrt(a2), "tile (%d, %d): %.3e", i, j, std::sqrt(e2 / a2));
            CHECK(std::fabs(w[0] - a2) <= 1e-10 * a2, "tile (%d, %d) err2[0]", i, j);
            CHECK(w[1] <= 1e-18 * a2, "tile (%d, %d) err2[1] %.3e", i, j, w[1]);
        }

    bool threw = false;  // a tile that does not divide the matrix is refused
    try {
        rsvd::compress(A, T, l, k, 30, 50);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    CHECK(threw, "30 x 50 tiles of a 100 x 100 matrix must throw std::invalid_argument");

    std::printf(fails ? "FAILED (%d)\n" : "PASSED\n", fails);
    return fails ? 1 : 0;
}
