// pod.cpp -- host side of the snapshot-method POD (include/rsvd_c.h, ABI 9; the reference's class POD,
// POD/ParametricDiffusion1D/src/POD.cpp:136-462, ns <= Nh branch): validation, the workspace layout and
// the launch sequence  T = Xh S  ->  C = D^1/2 S^T T D^1/2 (fp64)  ->  rsvd_svd / rsvd_run on C (fp64)
// ->  rank rule and Z = D^1/2 V diag(1 / sigma)  ->  W = S Z.  Nothing here synchronises.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/rsvd_c.h"
#include "dense.hpp"
#include "handle.hpp"
#include "pod.hpp"

using namespace rsvd;

namespace {

int check_pod(const rsvd_pod_desc_t* d, const char** err) {
    if (!d) { *err = "null descriptor"; return RSVD_ERR_INVALID_ARG; }
    if (d->nh < 1 || d->ns < 1) { *err = "S must have at least one row and one column"; return RSVD_ERR_INVALID_ARG; }
    if (d->r < 1 || d->r > d->ns) { *err = "r must be in 1 .. ns"; return RSVD_ERR_INVALID_ARG; }
    if (d->lds < d->nh) { *err = "lds < nh"; return RSVD_ERR_INVALID_ARG; }
    if (!(d->tol >= 0.0 && d->tol <= 1.0)) { *err = "tol must be in [0, 1]"; return RSVD_ERR_INVALID_ARG; }
    if (d->svd_type < 0 || d->svd_type > 5) { *err = "svd_type must be in 0 .. 5"; return RSVD_ERR_INVALID_ARG; }
    if (d->flags & ~RSVD_POD_FLAG_TEXTBOOK) { *err = "unknown flags"; return RSVD_ERR_INVALID_ARG; }
    if (d->q < 0) { *err = "q < 0"; return RSVD_ERR_INVALID_ARG; }
    if (d->dtype < RSVD_F64 || d->dtype > RSVD_FP8_E4M3) { *err = "unknown dtype"; return RSVD_ERR_INVALID_ARG; }
    if (d->ns > d->nh) {
        *err = "ns > nh (the reference's K = S S^T branch) is not supported";
        return RSVD_ERR_UNSUPPORTED;
    }
    if (d->ns > 4096) { *err = "ns > 4096"; return RSVD_ERR_UNSUPPORTED; }
    if (d->svd_type == 0 || d->svd_type == 3) {
        *err = "svd_type 0 / 3 (power method) is not supported by rsvd_pod";
        return RSVD_ERR_UNSUPPORTED;
    }
    if (d->dtype != RSVD_F64 && d->dtype != RSVD_F32) { *err = "S must be F64 or F32"; return RSVD_ERR_UNSUPPORTED; }
    return RSVD_OK;
}

bool direct_svd(const rsvd_pod_desc_t* d) { return d->svd_type == 1 || d->svd_type == 2; }
// svd_type 2 runs the converged Jacobi SVD as well.  rsvd_svd's ParallelJacobi is the reference's own
// iteration (SVD_class.hpp:223-333), which stops at an absolute weight of 1e-12 and leaves its vectors
// ~1e-5 from the SVD's (on C of a 1037 x 37 S: sigma off by 1.9e-9, W by 2.5e-5); the division by sigma_i
// hands that to the modes.  rsvd_run makes no such difference between the two (svd_type 4 / 5).
int method_of(const rsvd_pod_desc_t* d) {
    if (direct_svd(d)) return RSVD_SVD_JACOBI;
    return d->svd_type == 4 ? RSVD_SVD_JACOBI : RSVD_SVD_PARALLEL_JACOBI;
}

// rSVD(C, U, sigma, V, r, method) of POD.cpp:72-84 on the fp64 C
rsvd_desc_t nested_desc(const rsvd_pod_desc_t* d) {
    rsvd_desc_t nd{};
    nd.m = nd.n = nd.lda = d->ns;
    nd.l = d->r;
    nd.q = d->q;
    nd.dtype = RSVD_F64;
    nd.method = method_of(d);
    nd.qr_mode = RSVD_QR_AUTO;
    nd.seed = d->seed;
    return nd;
}

// POD's own region (T, the slabs, C, the small factors, Z), then what the nested solver needs.
struct PodWs {
    PodPlan plan;
    int kf;  // columns of the small factors: ns (svd_type 1 / 2) or r
    size_t oT, oSlab, oC, oU, oV, oZ, own, total;
};

int plan_ws(const rsvd_pod_desc_t* d, bool has_xh, PodWs* w) {
    const size_t es = d->dtype == RSVD_F64 ? 8 : 4;
    const size_t ns = (size_t)d->ns;
    w->plan = plan_pod_corr(d->nh, d->ns, d->dtype);
    w->kf = direct_svd(d) ? (int)d->ns : d->r;
    w->oT = 0;
    w->oSlab = w->oT + (has_xh ? align256(sizeof(double) * (size_t)d->nh * ns) : 0);  // T = Xh S stays fp64
    w->oC = w->oSlab + align256(pod_slab_bytes(w->plan));
    w->oU = w->oC + align256(sizeof(double) * ns * ns);
    w->oV = w->oU + align256(sizeof(double) * ns * w->kf);
    w->oZ = w->oV + align256(sizeof(double) * ns * w->kf);
    w->own = w->oZ + align256(es * ns * d->r);
    size_t nested = 0;
    if (direct_svd(d)) {
        RSVD_TRY(rsvd_svd_workspace_bytes(d->ns, d->ns, RSVD_F64, method_of(d), &nested));
    } else {
        const rsvd_desc_t nd = nested_desc(d);
        RSVD_TRY(rsvd_workspace_bytes(&nd, &nested));
    }
    w->total = w->own + align256(nested);
    return RSVD_OK;
}

// The nested rsvd_svd / rsvd_run sees the tail of the workspace as a caller-owned one of its own.
struct WsWindow {
    rsvd_handle_t h;
    char* ws;
    size_t bytes;
    bool ext;
    WsWindow(rsvd_handle_t h_, size_t off) : h(h_), ws(h_->ws), bytes(h_->ws_bytes), ext(h_->ws_external) {
        h->ws = ws + off;
        h->ws_bytes = bytes - off;
        h->ws_external = true;
    }
    ~WsWindow() {
        h->ws = ws;
        h->ws_bytes = bytes;
        h->ws_external = ext;
    }
};

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

extern "C" {

int rsvd_pod_workspace_bytes(const rsvd_pod_desc_t* d, int has_xh, size_t* bytes) {
    if (!bytes) return RSVD_ERR_INVALID_ARG;
    const char* err = "";
    RSVD_TRY(check_pod(d, &err));
    PodWs w;
    RSVD_TRY(plan_ws(d, has_xh != 0, &w));
    *bytes = w.total;
    return RSVD_OK;
}

int rsvd_pod_plan(const rsvd_pod_desc_t* d, int32_t* tiles, int32_t* chunks) {
    if (!tiles || !chunks) return RSVD_ERR_INVALID_ARG;
    const char* err = "";
    RSVD_TRY(check_pod(d, &err));
    const PodPlan p = plan_pod_corr(d->nh, d->ns, d->dtype);
    *tiles = p.blocks;
    *chunks = p.chunks;
    return RSVD_OK;
}

int rsvd_pod(rsvd_handle_t h, const rsvd_pod_desc_t* d, const void* S, const rsvd_csr_t* Xh, const double* dw, void* W,
             int64_t ldw, double* sigma, int32_t* N, double* C) {
    if (!h) return RSVD_ERR_INVALID_ARG;
    const char* err = "";
    const int st = check_pod(d, &err);
    if (st != RSVD_OK) {
        h->err = err;
        return st;
    }
    if (!S || !W || !sigma || !N || ldw < d->nh) {
        h->err = "null pointer or ldw < nh";
        return RSVD_ERR_INVALID_ARG;
    }
    if (Xh && (Xh->nnz < 0 || !Xh->rowptr || (Xh->nnz > 0 && (!Xh->colind || !Xh->val)))) {
        h->err = "bad CSR matrix (nnz < 0 or null arrays)";
        return RSVD_ERR_INVALID_ARG;
    }
    if (h->world > 1) {
        h->err = "POD is single-GPU (the handle is row-sharded)";
        return RSVD_ERR_UNSUPPORTED;
    }
    RSVD_CK(hipSetDevice(h->device));
    PodWs w;
    RSVD_TRY(plan_ws(d, Xh != nullptr, &w));
    RSVD_TRY(ensure_ws(h, w.total));
    char* ws = h->ws;
    const int dt = d->dtype == RSVD_F64 ? 0 : 1;
    const int64_t nh = d->nh, ns = d->ns;
    const void* T = S;
    int64_t ldt = d->lds;
    if (Xh) {
        RSVD_CK(launch_pod_spmm(dt, Xh->rowptr, Xh->colind, Xh->val, Xh->nnz, nh, ns, S, d->lds,
                                reinterpret_cast<double*>(ws + w.oT), h->stream));
        T = ws + w.oT;
        ldt = nh;
    }
    double* Cw = reinterpret_cast<double*>(ws + w.oC);
    double* Uw = reinterpret_cast<double*>(ws + w.oU);
    double* Vw = reinterpret_cast<double*>(ws + w.oV);
    RSVD_CK(launch_pod_corr(dt, S, d->lds, T, Xh != nullptr, ldt, nh, ns, w.plan, dw,
                            reinterpret_cast<double*>(ws + w.oSlab), Cw, C, h->stream));
    {
        WsWindow win(h, w.own);
        if (direct_svd(d)) {
            int32_t kept = 0;
            RSVD_TRY(rsvd_svd(h, ns, ns, Cw, ns, RSVD_F64, method_of(d), 0, 0, Uw, ns, sigma, Vw, ns, &kept));
        } else {
            const rsvd_desc_t nd = nested_desc(d);
            RSVD_TRY(rsvd_run(h, &nd, Cw, nullptr, 0, Uw, ns, sigma, Vw, ns));
        }
    }
    RSVD_CK(launch_pod_finish(dt, Vw, ns, (int)ns, d->r, w.kf, dw, d->tol, d->flags & RSVD_POD_FLAG_TEXTBOOK, sigma, N,
                              ws + w.oZ, h->stream));
    // the lift W = S Z (nh x ns times ns x r); beta = 0 never reads W, rows nh .. ldw are not touched
    if (dt == 0)
        RSVD_CK(launch_gemm<double>(0, 0, nh, d->r, ns, 1.0, static_cast<const double*>(S), d->lds,
                                    reinterpret_cast<const double*>(ws + w.oZ), ns, 0.0, static_cast<double*>(W), ldw,
                                    h->stream));
    else
        RSVD_CK(launch_gemm<float>(0, 0, nh, d->r, ns, 1.f, static_cast<const float*>(S), d->lds,
                                   reinterpret_cast<const float*>(ws + w.oZ), ns, 0.f, static_cast<float*>(W), ldw,
                                   h->stream));
    return RSVD_OK;
}

int rsvd_pod_host_f64(rsvd_handle_t h, const rsvd_pod_desc_t* desc, const double* S, const int32_t* rowptr,
                      const int32_t* colind, const double* val, int64_t nnz, const double* dw, double* W, double* sigma,
                      int32_t* N) {
    if (!h) return RSVD_ERR_INVALID_ARG;
    const char* err = "";
    if (!desc) return RSVD_ERR_INVALID_ARG;
    rsvd_pod_desc_t d = *desc;
    d.dtype = RSVD_F64;
    const int st = check_pod(&d, &err);
    if (st != RSVD_OK) {
        h->err = err;
        return st;
    }
    if (!S || !W || !sigma || !N || (rowptr && (nnz < 0 || (nnz > 0 && (!colind || !val))))) {
        h->err = "null pointer or nnz < 0";
        return RSVD_ERR_INVALID_ARG;
    }
    RSVD_CK(hipSetDevice(h->device));
    const int64_t nh = d.nh, ns = d.ns;
    DevBuf dS, dRp, dCi, dVal, dD, dWm, dSig, dN;
    RSVD_CK(hipMalloc(&dS.p, sizeof(double) * nh * ns));
    RSVD_CK(hipMalloc(&dWm.p, sizeof(double) * nh * d.r));
    RSVD_CK(hipMalloc(&dSig.p, sizeof(double) * ns));
    RSVD_CK(hipMalloc(&dN.p, sizeof(int32_t)));
    RSVD_CK(hipMemcpy2DAsync(dS.p, sizeof(double) * nh, S, sizeof(double) * d.lds, sizeof(double) * nh, ns,
                             hipMemcpyHostToDevice, h->stream));
    rsvd_csr_t X{};
    if (rowptr) {
        RSVD_CK(hipMalloc(&dRp.p, sizeof(int32_t) * (nh + 1)));
        RSVD_CK(hipMalloc(&dCi.p, sizeof(int32_t) * (nnz > 0 ? nnz : 1)));
        RSVD_CK(hipMalloc(&dVal.p, sizeof(double) * (nnz > 0 ? nnz : 1)));
        RSVD_CK(hipMemcpyAsync(dRp.p, rowptr, sizeof(int32_t) * (nh + 1), hipMemcpyHostToDevice, h->stream));
        if (nnz > 0) {
            RSVD_CK(hipMemcpyAsync(dCi.p, colind, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, h->stream));
            RSVD_CK(hipMemcpyAsync(dVal.p, val, sizeof(double) * nnz, hipMemcpyHostToDevice, h->stream));
        }
        X.rowptr = static_cast<const int32_t*>(dRp.p);
        X.colind = static_cast<const int32_t*>(dCi.p);
        X.val = dVal.p;
        X.nnz = nnz;
    }
    if (dw) {
        RSVD_CK(hipMalloc(&dD.p, sizeof(double) * ns));
        RSVD_CK(hipMemcpyAsync(dD.p, dw, sizeof(double) * ns, hipMemcpyHostToDevice, h->stream));
    }
    d.lds = nh;
    const int run = rsvd_pod(h, &d, dS.p, rowptr ? &X : nullptr, static_cast<const double*>(dD.p), dWm.p, nh,
                             static_cast<double*>(dSig.p), static_cast<int32_t*>(dN.p), nullptr);
    if (run != RSVD_OK) {
        (void)hipStreamSynchronize(h->stream);  // the buffers above are freed on return
        return run;
    }
    RSVD_CK(hipMemcpyAsync(W, dWm.p, sizeof(double) * nh * d.r, hipMemcpyDeviceToHost, h->stream));
    RSVD_CK(hipMemcpyAsync(sigma, dSig.p, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    RSVD_CK(hipMemcpyAsync(N, dN.p, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    return rsvd_sync(h);
}

}  // extern "C"
