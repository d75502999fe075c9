// batched_run.cpp -- host side of the batched rSVD (include/rsvd_c.h, ABI 7) and of the rank-k
// compression on top of it (ABI 8): validation, the choice between the fused kernel (batched.hip: one
// workgroup per matrix, one launch) and the loop of rsvd_run (+ rsvd_lowrank) over the sub-pointers,
// and the workspace arithmetic of both.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/rsvd_c.h"
#include "batched.hpp"
#include "handle.hpp"
#include "lowrank.hpp"

using namespace rsvd;

namespace {

// The descriptor checks of rsvd_run (through rsvd_workspace_bytes, which needs no handle) plus the
// batch's own.  ldu / ldv = 0: not known (a workspace query): the outputs' smallest footprints count.
// factors = false (a compress call without U, S, V): the output strides are not looked at.
int check_batch(const rsvd_desc_t* d, const rsvd_batch_t* bt, int64_t ldu, int64_t ldv, const char** err,
                bool factors = true) {
    if (!d || !bt) { *err = "null descriptor"; return RSVD_ERR_INVALID_ARG; }
    size_t one = 0;
    const int st = rsvd_workspace_bytes(d, &one);
    if (st != RSVD_OK) { *err = "invalid matrix description"; return st; }
    if (d->flags != 0) { *err = "batched runs take no flags"; return RSVD_ERR_INVALID_ARG; }
    if (d->method == RSVD_SVD_POWER || d->method == RSVD_SVD_POWER_IC) {
        *err = "the power-method small SVD is not available in batches";
        return RSVD_ERR_UNSUPPORTED;
    }
    if (bt->count0 < 1 || bt->count1 < 1) { *err = "batch counts must be >= 1"; return RSVD_ERR_INVALID_ARG; }
    if (bt->a_stride0 < 0 || bt->a_stride1 < 0 || bt->omega_stride < 0 ||
        (factors && (bt->u_stride < 0 || bt->s_stride < 0 || bt->v_stride < 0))) {
        *err = "negative batch stride";
        return RSVD_ERR_INVALID_ARG;
    }
    if (!factors) return RSVD_OK;
    if (ldu == 0) ldu = d->m;
    if (ldv == 0) ldv = d->n;
    if (ldu < d->m || ldv < d->n) { *err = "bad leading dimension"; return RSVD_ERR_INVALID_ARG; }
    if (bt->u_stride < ldu * d->l || bt->s_stride < d->l || bt->v_stride < ldv * d->l) {
        *err = "an output stride is smaller than the output (ldu * l, l, ldv * l)";
        return RSVD_ERR_INVALID_ARG;
    }
    return RSVD_OK;
}

bool fused_limits(const rsvd_desc_t* d) {
    return (d->dtype == RSVD_F64 || d->dtype == RSVD_F32) && d->l >= 1 && d->l <= kBatchedMaxL && d->l <= d->m &&
           d->l <= d->n && d->m <= kBatchedMaxDim && d->n <= kBatchedMaxDim && d->q >= 0 &&
           (d->method == RSVD_SVD_JACOBI || d->method == RSVD_SVD_PARALLEL_JACOBI) && d->qr_mode == RSVD_QR_AUTO &&
           d->flags == 0;
}

struct FusedPlan {
    int LP, grid;
    bool plds;
    size_t lds, slice, ws;
};

FusedPlan plan_fused(const rsvd_desc_t* d, int64_t batch) {
    FusedPlan p;
    p.LP = lp_of(d->l);
    const size_t small = batched_small_bytes(d->dtype, p.LP);
    const size_t panels = batched_panel_bytes(d->dtype, (int)d->m, (int)d->n, d->l);
    p.plds = small + panels <= kBatchedLdsBudget;
    p.lds = p.plds ? small + panels : small;
    p.grid = (int)std::min<int64_t>(batch, kBatchedMaxGrid);
    p.slice = p.plds ? 0 : panels;
    p.ws = std::max<size_t>(p.slice * p.grid, 256);
    return p;
}

size_t in_bytes(int dtype) { return dtype == RSVD_F64 ? 8 : dtype == RSVD_F32 ? 4 : dtype == RSVD_BF16 ? 2 : 1; }
size_t out_bytes(int dtype) { return dtype == RSVD_F64 ? 8 : 4; }

// count0 x count1 blocks of m x n at stride0 / stride1 inside leading dimension ld are pairwise disjoint
// for the two layouts the compression accepts: a tile grid (the blocks of a row of tiles share columns)
// or a strided batch (every block past the one before).  The stride of a dimension of one carries no
// meaning and is not looked at.
bool disjoint_blocks(int64_t c0, int64_t c1, int64_t s0, int64_t s1, int64_t m, int64_t n, int64_t ld) {
    const int64_t foot = (n - 1) * ld + m;
    const bool grid = (c0 == 1 || (s0 >= m && (c0 - 1) * s0 + m <= ld)) && (c1 == 1 || s1 >= n * ld);
    const bool strided = (c0 == 1 || s0 >= foot) && (c1 == 1 || s1 >= (c0 == 1 ? foot : c0 * s0));
    return grid || strided;
}

int check_comp(const rsvd_desc_t* d, const rsvd_batch_t* bt, const rsvd_compress_t* c, const char** err) {
    if (!c) { *err = "null compression description"; return RSVD_ERR_INVALID_ARG; }
    if (c->k < 1 || c->k > d->l || c->k > d->n) { *err = "k must be in 1 .. min(l, n)"; return RSVD_ERR_INVALID_ARG; }
    if (c->ldc < d->m) { *err = "ldc < m"; return RSVD_ERR_INVALID_ARG; }
    if (c->c_stride0 < 0 || c->c_stride1 < 0) { *err = "negative C stride"; return RSVD_ERR_INVALID_ARG; }
    if (!disjoint_blocks(bt->count0, bt->count1, c->c_stride0, c->c_stride1, d->m, d->n, c->ldc)) {
        *err = "the C blocks overlap (neither a tile grid nor a strided batch)";
        return RSVD_ERR_INVALID_ARG;
    }
    return RSVD_OK;
}

// Looped compress path: [0, base) is rsvd_run's workspace, reused for the error slots of rsvd_lowrank
// once the run is done with it; the factors of one matrix sit behind it when the caller passed none.
struct LoopPlan {
    size_t base, oU, oS, oV, total;
};

int plan_loop(const rsvd_desc_t* d, LoopPlan* p) {
    size_t run = 0;
    RSVD_TRY(rsvd_workspace_bytes(d, &run));
    const size_t ob = out_bytes(d->dtype);
    const size_t slots = sizeof(double) * 2 * (size_t)lowrank_tiles(d->m, d->n);
    p->base = align256(std::max(run, slots));
    p->oU = p->base;
    p->oS = p->oU + align256(ob * (size_t)d->m * d->l);
    p->oV = p->oS + align256(ob * (size_t)d->l);
    p->total = p->oV + align256(ob * (size_t)d->n * d->l);
    return RSVD_OK;
}

struct CompCall {  // what a compress call adds to a batched run
    const rsvd_compress_t* c;
    void* C;
    double* err2;
};

// rsvd_run_batched, and rsvd_compress_batched when cc is set (U, S, V may then be null together).
int run_batched(rsvd_handle_t h, const rsvd_desc_t* d, const rsvd_batch_t* bt, const void* A, const void* omega,
                int64_t ldo, void* U, int64_t ldu, void* S, void* V, int64_t ldv, int32_t* info, const CompCall* cc);

}  // namespace

extern "C" {

int rsvd_batched_is_fused(const rsvd_desc_t* d, const rsvd_batch_t* bt) {
    const char* err = "";
    if (check_batch(d, bt, 0, 0, &err) != RSVD_OK) return 0;
    return fused_limits(d) ? 1 : 0;
}

int rsvd_batched_workspace_bytes(const rsvd_desc_t* d, const rsvd_batch_t* bt, size_t* bytes) {
    if (!bytes) return RSVD_ERR_INVALID_ARG;
    const char* err = "";
    RSVD_TRY(check_batch(d, bt, 0, 0, &err));
    if (fused_limits(d)) {
        *bytes = plan_fused(d, bt->count0 * bt->count1).ws;
        return RSVD_OK;
    }
    return rsvd_workspace_bytes(d, bytes);
}

int rsvd_run_batched(rsvd_handle_t h, const rsvd_desc_t* d, const rsvd_batch_t* bt, const void* A, const void* omega,
                     int64_t ldo, void* U, int64_t ldu, void* S, void* V, int64_t ldv, int32_t* info) {
    if (!h) return RSVD_ERR_INVALID_ARG;
    if (!U || !S || !V) {
        h->err = "null pointer or bad leading dimension";
        return RSVD_ERR_INVALID_ARG;
    }
    return run_batched(h, d, bt, A, omega, ldo, U, ldu, S, V, ldv, info, nullptr);
}

int rsvd_compress_workspace_bytes(const rsvd_desc_t* d, const rsvd_batch_t* bt, const rsvd_compress_t* c,
                                  size_t* bytes) {
    if (!bytes) return RSVD_ERR_INVALID_ARG;
    const char* err = "";
    RSVD_TRY(check_batch(d, bt, 0, 0, &err, false));
    RSVD_TRY(check_comp(d, bt, c, &err));
    if (fused_limits(d)) {
        *bytes = plan_fused(d, bt->count0 * bt->count1).ws;
        return RSVD_OK;
    }
    LoopPlan lp;
    RSVD_TRY(plan_loop(d, &lp));
    *bytes = lp.total;
    return RSVD_OK;
}

int rsvd_compress_batched(rsvd_handle_t h, const rsvd_desc_t* d, const rsvd_batch_t* bt, const rsvd_compress_t* c,
                          const void* A, const void* omega, int64_t ldo, void* C, void* U, int64_t ldu, void* S, void* V,
                          int64_t ldv, double* err2, int32_t* info) {
    if (!h) return RSVD_ERR_INVALID_ARG;
    const bool any = U || S || V, all = U && S && V;
    if (any != all) {
        h->err = "U, S and V must be all set or all null";
        return RSVD_ERR_INVALID_ARG;
    }
    if (!C && !err2) {
        h->err = "nothing to compute: C and err2 are both null";
        return RSVD_ERR_INVALID_ARG;
    }
    const CompCall cc{c, C, err2};
    return run_batched(h, d, bt, A, omega, ldo, U, ldu, S, V, ldv, info, &cc);
}

int rsvd_lowrank_workspace_bytes(int64_t m, int64_t n, size_t* bytes) {
    if (!bytes || m < 1 || n < 1) return RSVD_ERR_INVALID_ARG;
    *bytes = align256(sizeof(double) * 2 * (size_t)lowrank_tiles(m, n));
    return RSVD_OK;
}

int rsvd_lowrank(rsvd_handle_t h, int64_t m, int64_t n, int32_t k, int32_t dtype, const void* U, int64_t ldu,
                 const void* S, const void* V, int64_t ldv, void* C, int64_t ldc, const void* A, int64_t lda,
                 int32_t a_dtype, double a_scale, double* err2) {
    if (!h) return RSVD_ERR_INVALID_ARG;
    if (m < 1 || n < 1 || k < 1 || !U || !S || !V || ldu < m || ldv < n || (C && ldc < m) || (A && lda < m) ||
        (!C && !(A && err2)) || (err2 && !A)) {
        h->err = "null pointer, bad size or bad leading dimension";
        return RSVD_ERR_INVALID_ARG;
    }
    if (k > 4096) {
        h->err = "k > 4096";
        return RSVD_ERR_UNSUPPORTED;
    }
    // C has the result type of A: fp64 for fp64 A, fp32 for every other A
    const bool f64 = dtype == RSVD_F64;
    if ((!f64 && dtype != RSVD_F32) || (A && err2 && (a_dtype < RSVD_F64 || a_dtype > RSVD_FP8_E4M3 ||
                                                      f64 != (a_dtype == RSVD_F64)))) {
        h->err = "dtype must be F64 (with F64 A) or F32 (with F32 / BF16 / FP8_E4M3 A)";
        return RSVD_ERR_INVALID_ARG;
    }
    RSVD_CK(hipSetDevice(h->device));
    double* slots = nullptr;
    if (A && err2) {
        size_t bytes = 0;
        RSVD_TRY(rsvd_lowrank_workspace_bytes(m, n, &bytes));
        RSVD_TRY(ensure_ws(h, bytes));
        slots = reinterpret_cast<double*>(h->ws);
    }
    RSVD_CK(launch_lowrank(f64 ? 0 : 1, m, n, k, U, ldu, S, V, ldv, C, ldc, A, lda, a_dtype,
                           a_scale != 0.0 ? a_scale : 1.0, slots, err2, h->stream));
    return RSVD_OK;
}

namespace {
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};
}  // namespace

int rsvd_compress_host_f64(rsvd_handle_t h, int64_t m, int64_t n, const double* A, int64_t lda, int32_t tile_m,
                           int32_t tile_n, int32_t l, int32_t k, int32_t q, uint64_t seed, double* C, int64_t ldc,
                           double* err2) {
    if (!h) return RSVD_ERR_INVALID_ARG;
    if (tile_m == 0 && tile_n == 0) {
        tile_m = (int32_t)m;
        tile_n = (int32_t)n;
    }
    if (!A || !C || m < 1 || n < 1 || lda < m || ldc < m || tile_m < 1 || tile_n < 1 || m % tile_m || n % tile_n) {
        h->err = "null pointer, bad leading dimension or a tile that does not divide the matrix";
        return RSVD_ERR_INVALID_ARG;
    }
    rsvd_desc_t d{};
    d.m = tile_m; d.n = tile_n; d.lda = m; d.l = l; d.q = q; d.dtype = RSVD_F64; d.method = RSVD_SVD_JACOBI;
    d.qr_mode = RSVD_QR_AUTO; d.seed = seed;
    rsvd_batch_t bt{};
    bt.count0 = m / tile_m; bt.count1 = n / tile_n; bt.a_stride0 = tile_m; bt.a_stride1 = (int64_t)tile_n * m;
    rsvd_compress_t c{};
    c.k = k; c.ldc = m; c.c_stride0 = bt.a_stride0; c.c_stride1 = bt.a_stride1;
    const int64_t tiles = bt.count0 * bt.count1;
    RSVD_CK(hipSetDevice(h->device));
    DevBuf dA, dE;  // compressed in place on the device copy, as image_matrix.block(...) = localMatrix
    RSVD_CK(hipMalloc(&dA.p, sizeof(double) * m * n));
    RSVD_CK(hipMalloc(&dE.p, sizeof(double) * 2 * tiles));
    RSVD_CK(hipMemcpy2DAsync(dA.p, sizeof(double) * m, A, sizeof(double) * lda, sizeof(double) * m, n,
                             hipMemcpyHostToDevice, h->stream));
    RSVD_TRY(rsvd_compress_batched(h, &d, &bt, &c, dA.p, nullptr, 0, dA.p, nullptr, 0, nullptr, nullptr, 0,
                                   static_cast<double*>(dE.p), nullptr));
    RSVD_CK(hipMemcpy2DAsync(C, sizeof(double) * ldc, dA.p, sizeof(double) * m, sizeof(double) * m, n,
                             hipMemcpyDeviceToHost, h->stream));
    if (err2) RSVD_CK(hipMemcpyAsync(err2, dE.p, sizeof(double) * 2 * tiles, hipMemcpyDeviceToHost, h->stream));
    return rsvd_sync(h);
}

}  // extern "C"

namespace {

int run_batched(rsvd_handle_t h, const rsvd_desc_t* d, const rsvd_batch_t* bt, const void* A, const void* omega,
                int64_t ldo, void* U, int64_t ldu, void* S, void* V, int64_t ldv, int32_t* info, const CompCall* cc) {
    const char* err = "";
    const bool factors = U != nullptr;
    if (factors && (ldu <= 0 || ldv <= 0)) {
        h->err = "null pointer or bad leading dimension";
        return RSVD_ERR_INVALID_ARG;
    }
    int st = check_batch(d, bt, ldu, ldv, &err, factors);
    if (st == RSVD_OK && cc) st = check_comp(d, bt, cc->c, &err);
    if (st == RSVD_OK && cc && cc->C == A &&
        !((d->dtype == RSVD_F64 || d->dtype == RSVD_F32) && cc->c->ldc == d->lda &&
          (bt->count0 == 1 || cc->c->c_stride0 == bt->a_stride0) &&
          (bt->count1 == 1 || cc->c->c_stride1 == bt->a_stride1))) {
        err = "in place needs A of C's type, ldc == lda and the strides of A";
        st = RSVD_ERR_INVALID_ARG;
    }
    if (st != RSVD_OK) {
        h->err = err;
        return st;
    }
    if (h->world > 1) {
        h->err = "batched runs are single-GPU (the handle is row-sharded)";
        return RSVD_ERR_UNSUPPORTED;
    }
    if (!A || (omega && ldo < d->n)) {
        h->err = "null pointer or bad leading dimension";
        return RSVD_ERR_INVALID_ARG;
    }
    RSVD_CK(hipSetDevice(h->device));
    const int64_t batch = bt->count0 * bt->count1;
    const double sc = d->a_scale != 0.0 ? d->a_scale : 1.0;
    if (fused_limits(d)) {
        const FusedPlan p = plan_fused(d, batch);
        RSVD_TRY(ensure_ws(h, p.ws));
        RSVD_CK(reset_run_flags(h->dflags, h->stream));
        BatchedArgs a{};
        a.A = A; a.omega = omega; a.U = U; a.S = S; a.V = V; a.info = info;
        a.nonfinite = h->dflags + kFlagNonFinite;
        a.ws = h->ws; a.ws_slice = p.slice;
        a.batch = batch; a.count0 = bt->count0; a.a_stride0 = bt->a_stride0; a.a_stride1 = bt->a_stride1;
        a.omega_stride = bt->omega_stride; a.u_stride = bt->u_stride; a.s_stride = bt->s_stride;
        a.v_stride = bt->v_stride;
        a.lda = d->lda; a.ldo = ldo; a.ldu = ldu; a.ldv = ldv;
        a.m = (int)d->m; a.n = (int)d->n; a.l = d->l; a.q = d->q;
        a.seed = d->seed; a.s_scale = std::fabs(sc); a.v_neg = sc < 0.0;
        if (cc) {
            a.C = cc->C; a.err2 = cc->err2; a.k = cc->c->k; a.ldc = cc->c->ldc;
            a.c_stride0 = cc->c->c_stride0; a.c_stride1 = cc->c->c_stride1;
            RSVD_CK(launch_batched_compress(a, d->dtype, p.LP, p.plds, p.lds, p.grid, h->stream));
        } else {
            RSVD_CK(launch_batched_rsvd(a, d->dtype, p.LP, p.plds, p.lds, p.grid, h->stream));
        }
        return RSVD_OK;
    }
    // Outside the fused limits: rsvd_run (then rsvd_lowrank's kernels) per matrix on the same stream, seed + b.
    const size_t ib = in_bytes(d->dtype), ob = out_bytes(d->dtype);
    int64_t u_stride = bt->u_stride, s_stride = bt->s_stride, v_stride = bt->v_stride;
    LoopPlan lp{};
    if (cc) {
        RSVD_TRY(plan_loop(d, &lp));
        RSVD_TRY(ensure_ws(h, lp.total));
        if (!factors) {  // one matrix's factors, behind what rsvd_run uses of the workspace
            U = h->ws + lp.oU; S = h->ws + lp.oS; V = h->ws + lp.oV;
            ldu = d->m; ldv = d->n;
            u_stride = s_stride = v_stride = 0;
        }
    }
    std::vector<int32_t> hinfo(info ? 2 * batch : 0);
    bool nonfinite = false;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t i0 = b % bt->count0, i1 = b / bt->count0;
        rsvd_desc_t db = *d;
        db.seed = d->seed + (uint64_t)b;
        const char* Ab = static_cast<const char*>(A) + ib * (size_t)(i0 * bt->a_stride0 + i1 * bt->a_stride1);
        const char* Ob = omega ? static_cast<const char*>(omega) + ob * (size_t)(b * bt->omega_stride) : nullptr;
        char* Ub = static_cast<char*>(U) + ob * (size_t)(b * u_stride);
        char* Sb = static_cast<char*>(S) + ob * (size_t)(b * s_stride);
        char* Vb = static_cast<char*>(V) + ob * (size_t)(b * v_stride);
        RSVD_TRY(rsvd_run(h, &db, Ab, Ob, ldo, Ub, ldu, Sb, Vb, ldv));
        if (cc) {
            char* Cb = cc->C ? static_cast<char*>(cc->C) + ob * (size_t)(i0 * cc->c->c_stride0 + i1 * cc->c->c_stride1)
                             : nullptr;
            RSVD_CK(launch_lowrank(d->dtype == RSVD_F64 ? 0 : 1, d->m, d->n, cc->c->k, Ub, ldu, Sb, Vb, ldv, Cb,
                                   cc->c->ldc, Ab, d->lda, d->dtype, sc, reinterpret_cast<double*>(h->ws),
                                   cc->err2 ? cc->err2 + 2 * b : nullptr, h->stream));
        }
        if (info) {  // the handle's per-run diagnostics: one synchronisation per matrix
            int flags[kFlagWords] = {0};
            RSVD_CK(hipMemcpyAsync(flags, h->dflags, sizeof(flags), hipMemcpyDeviceToHost, h->stream));
            RSVD_CK(hipStreamSynchronize(h->stream));
            int fallbacks = 0;
            for (int k = 4; k < 16; ++k) fallbacks += flags[k] != 0;
            const bool nf = flags[kFlagNonFinite] != 0;
            hinfo[2 * b] = flags[1];
            hinfo[2 * b + 1] = (fallbacks ? 1 : 0) | (nf ? 2 : 0);
            if (nf) {  // give the later matrices a clean word; the sticky state is restored below
                nonfinite = true;
                RSVD_CK(hipMemsetAsync(h->dflags + kFlagNonFinite, 0, sizeof(int), h->stream));
            }
        }
    }
    if (info) {
        if (nonfinite) RSVD_CK(hipMemsetAsync(h->dflags + kFlagNonFinite, 1, sizeof(int), h->stream));
        RSVD_CK(hipMemcpyAsync(info, hinfo.data(), sizeof(int32_t) * hinfo.size(), hipMemcpyHostToDevice, h->stream));
        RSVD_CK(hipStreamSynchronize(h->stream));
    }
    return RSVD_OK;
}

}  // namespace
