// pod_test.cpp -- include/POD.hpp with the reference's call shapes (POD.hpp:24-49) on a known answer:
// S(i, j) = s_j delta_ij on 64 x 6 with distinct s, so C = diag(s^2), sigma = sort(s^2) and
// W[:, i] = +-e_pi(i) / s_pi(i).  Compiled by tests/test_cpp_pod.py against the Eigen stand-in.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "POD.hpp"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

// the reference's rule, POD.cpp:203-216
static int rank_rule(const std::vector<double> &sg, int r, double tol) {
    int N = 0;
    double I = 0.0, num = 0.0, den = 0.0;
    for (int i = 0; i < r; ++i) den += sg[i] * sg[i];
    while (I < (1 - tol * tol) && N < r) {
        num += sg[N] * sg[N];
        I = num / den;
        N++;
    }
    return N;
}

// sigma = scale s^2 (sorted), W[:, i] = +-wnum e_pi(i) / (scale s_pi(i))
static void check_modes(const POD &p, const std::vector<double> &s, double scale, double wnum, int r, double tol) {
    const int nh = 64, ns = (int)s.size();
    std::vector<int> order(ns);
    for (int j = 0; j < ns; ++j) order[j] = j;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return s[a] > s[b]; });
    std::vector<double> sg(ns);
    for (int i = 0; i < ns; ++i) sg[i] = scale * s[order[i]] * s[order[i]];
    EXPECT(p.sigma.size() == ns);
    for (int i = 0; i < ns; ++i) EXPECT(std::fabs(p.sigma(i) - sg[i]) <= 1e-12 * sg[0]);
    const int N = rank_rule(sg, r, tol);
    EXPECT(N > 0 && N < r);
    EXPECT(p.W.rows() == nh && p.W.cols() == N);
    for (int i = 0; i < (int)p.W.cols(); ++i)
        for (int k = 0; k < nh; ++k) {
            const double want = k == order[i] ? wnum / (scale * s[order[i]]) : 0.0;
            EXPECT(std::fabs(std::fabs(p.W(k, i)) - want) <= 1e-12 * std::max(1.0, want));
        }
}

int main() {
    const int nh = 64, ns = 6, r = 6;
    const double tol = 0.3;
    const std::vector<double> s = {1.5, 3.0, 0.75, 2.25, 0.5, 1.0};
    Mat_m S(nh, ns);
    for (int j = 0; j < ns; ++j) S(j, j) = s[j];

    for (int svd_type : {1, 2, 4, 5}) {
        POD standard(S, r, tol, svd_type);
        check_modes(standard, s, 1.0, 1.0, r, tol);
    }

    Mat_m Xh(nh, nh);
    for (int i = 0; i < nh; ++i) Xh(i, i) = 2.0;
    POD energy(S, Xh, r, tol, 1);
    check_modes(energy, s, 2.0, 1.0, r, tol);

    Mat_m D(ns, ns);
    for (int j = 0; j < ns; ++j) D(j, j) = 0.1;  // Diff1D_openmp.cpp:229-231
    POD weight(S, Xh, D, r, tol, 1);
    check_modes(weight, s, 2.0 * 0.1, std::sqrt(0.1), r, tol);  // D^1/2 enters W once, sigma twice

    bool threw = false;
    D(0, 1) = 0.5;
    try {
        POD bad(S, Xh, D, r, tol, 1);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    EXPECT(threw);

    threw = false;
    Mat_m wide(4, 6);
    try {
        POD bad(wide, 2, tol, 1);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    EXPECT(threw);

    threw = false;
    try {
        POD bad(S, r, tol, 3);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    EXPECT(threw);

    threw = false;
    try {
        POD bad(S, r, tol, 6);
    } catch (const std::exception &) {
        threw = true;
    }
    EXPECT(threw);

    // the naive constructor is rSVD() on S (r = ns: the sketch spans the range whatever Omega was drawn)
    POD naive(S, r, 4);
    Mat_m U, V;
    Vec_v sig;
    rSVD(S, U, sig, V, r, SVDMethod::Jacobi);
    EXPECT(naive.W.rows() == U.rows() && naive.W.cols() == U.cols() && naive.sigma.size() == sig.size());
    for (int i = 0; i < (int)sig.size(); ++i) EXPECT(std::fabs(naive.sigma(i) - sig(i)) <= 1e-12 * sig(0));
    for (int j = 0; j < (int)U.cols(); ++j)
        for (int i = 0; i < (int)U.rows(); ++i) EXPECT(std::fabs(std::fabs(naive.W(i, j)) - std::fabs(U(i, j))) <= 1e-10);

    POD empty;
    EXPECT(empty.W.size() == 0);

    if (failures) std::printf("FAILED (%d)\n", failures);
    else std::printf("PASSED\n");
    return failures ? 1 : 0;
}
