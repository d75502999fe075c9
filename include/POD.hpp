// POD.hpp -- drop-in replacement for the reference's POD/ParametricDiffusion1D/src/POD.hpp (class POD
// with the same public members and constructors, POD.hpp:24-49), backed by the MI355X engine.
//
//   POD();                                                                          POD.hpp:28
//   POD(Mat_m &S, const int r, const int svd_type);                       naive     POD.hpp:31
//   POD(Mat_m &S, const int r, const double tol, const int svd_type);     standard  POD.hpp:34
//   POD(Mat_m &S, Mat_m &Xh, const int r, const double tol, const int svd_type);    POD.hpp:37  (energy)
//   POD(Mat_m &S, Mat_m &Xh, Mat_m &D, const int r, const double tol, const int svd_type);  :40 (weight)
//   Mat_m W;  Vec_v sigma;                                                          POD.hpp:46, :49
//
// The naive constructor is perform_SVD (POD.cpp:42-114) on S through include/SVD_class.hpp and
// include/rSVD.hpp.  The other three run the snapshot method (the ns <= Nh branch of POD.cpp:136-462) on the
// device through rsvd_pod_host_f64: the fp64 correlation matrix C = D^1/2 S^T Xh S D^1/2, its SVD
// (svd_type 1, 2) or rSVD (4, 5), the rank rule of POD.cpp:203-216 and W = S D^1/2 V diag(1 / sigma), cut
// to its first N columns (the reference's conservativeResize).  sigma has ns entries (the first r written
// for svd_type 4 / 5, zeros behind).  A dense Xh is converted to CSR here (exact zeros dropped); D must be
// diagonal.  std::invalid_argument: ns > Nh (the reference's K = S S^T, matrix-square-root and CG
// branches), svd_type 0 / 3 outside the naive constructor, a non-diagonal D, a svd_type outside 0..5
// (the reference prints and calls std::exit).  Nothing is printed.
//
// Uses only <Eigen/Dense> (rows, cols, data, resize, operator()).  Link with -lrsvd_hip.
#ifndef POD_H
#define POD_H

#include <Eigen/Dense>

#include <cstdint>
#include <stdexcept>
#include <vector>

#include "SVD_class.hpp"
#include "rSVD.hpp"

class POD {
public:
    POD() {}

    POD(Mat_m &S, const int r, const int svd_type) { naive_POD(S, r, svd_type); }

    POD(Mat_m &S, const int r, const double tol, const int svd_type) { snapshot_POD(S, nullptr, nullptr, r, tol, svd_type); }

    POD(Mat_m &S, Mat_m &Xh, const int r, const double tol, const int svd_type) {
        snapshot_POD(S, &Xh, nullptr, r, tol, svd_type);
    }

    POD(Mat_m &S, Mat_m &Xh, Mat_m &D, const int r, const double tol, const int svd_type) {
        snapshot_POD(S, &Xh, &D, r, tol, svd_type);
    }

    // Matrix containing the POD modes
    Mat_m W;

    // Vector containing the singular values
    Vec_v sigma;

private:
    static void check_type(const int svd_type) {
        if (svd_type < 0 || svd_type > 5) throw std::invalid_argument("The svd_type should be in [0,5].");
    }

    template <SVDMethod M>
    void dense_SVD(Mat_m &A, const int r) {
        SVD<M> svd(A, M == SVDMethod::Power ? r : 0);
        svd.compute();
        W = svd.getU();
        sigma = svd.getS();
    }

    // perform_SVD on S itself (POD.cpp:116-133)
    void naive_POD(Mat_m &S, const int r, const int svd_type) {
        check_type(svd_type);
        Mat_m V;
        switch (svd_type) {
            case 0: dense_SVD<SVDMethod::Power>(S, r); break;
            case 1: dense_SVD<SVDMethod::Jacobi>(S, r); break;
            case 2: dense_SVD<SVDMethod::ParallelJacobi>(S, r); break;
            case 3: rSVD(S, W, sigma, V, r, SVDMethod::Power); break;
            case 4: rSVD(S, W, sigma, V, r, SVDMethod::Jacobi); break;
            default: rSVD(S, W, sigma, V, r, SVDMethod::ParallelJacobi); break;
        }
    }

    void snapshot_POD(Mat_m &S, Mat_m *Xh, Mat_m *D, const int r, const double tol, const int svd_type) {
        check_type(svd_type);
        const int64_t nh = S.rows(), ns = S.cols();
        if (ns > nh) throw std::invalid_argument("POD: ns > Nh is not supported");
        if (svd_type == 0 || svd_type == 3) throw std::invalid_argument("POD: svd_type 0 / 3 (power method) is not supported");
        std::vector<int32_t> rowptr, colind;
        std::vector<double> val, d;
        if (Xh) {
            if (Xh->rows() != nh || Xh->cols() != nh) throw std::invalid_argument("POD: Xh must be Nh x Nh");
            rowptr.assign((size_t)nh + 1, 0);
            for (int64_t i = 0; i < nh; ++i) {
                for (int64_t j = 0; j < nh; ++j) {
                    const double x = (*Xh)(i, j);
                    if (x != 0.0) {
                        colind.push_back((int32_t)j);
                        val.push_back(x);
                    }
                }
                rowptr[(size_t)i + 1] = (int32_t)colind.size();
            }
        }
        if (D) {
            if (D->rows() != ns || D->cols() != ns) throw std::invalid_argument("POD: D must be ns x ns");
            d.resize((size_t)ns);
            for (int64_t j = 0; j < ns; ++j)
                for (int64_t i = 0; i < ns; ++i) {
                    if (i == j) d[(size_t)j] = (*D)(i, j);
                    else if ((*D)(i, j) != 0.0) throw std::invalid_argument("POD: only a diagonal D is supported");
                }
        }
        rsvd::Context &c = rsvd::Context::instance();
        rsvd_pod_desc_t desc{};
        desc.nh = nh;
        desc.ns = ns;
        desc.lds = nh;
        desc.r = r;
        desc.dtype = RSVD_F64;
        desc.svd_type = svd_type;
        desc.q = 2;  // src/rSVD.cpp:83
        desc.seed = (svd_type == 4 || svd_type == 5) ? c.next_seed() : 0;
        desc.tol = tol;
        Mat_m Wall;
        if (r >= 1) Wall.resize(nh, r);
        sigma.resize(ns);
        int32_t N = 0;
        rsvd::check(rsvd_pod_host_f64(c.handle(), &desc, S.data(), Xh ? rowptr.data() : nullptr, colind.data(), val.data(),
                                      (int64_t)val.size(), D ? d.data() : nullptr, Wall.data(), sigma.data(), &N),
                    "POD");
        W.resize(nh, N);
        for (int64_t j = 0; j < N; ++j)
            for (int64_t i = 0; i < nh; ++i) W(i, j) = Wall(i, j);
    }
};

#endif
