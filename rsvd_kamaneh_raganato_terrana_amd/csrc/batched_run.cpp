// batched_run.cpp -- host side of the batched rSVD (include/rsvd_c.h, ABI 7): validation, the choice
// between the fused kernel (batched.hip: one workgroup per matrix, one launch) and the loop of
// rsvd_run over the sub-pointers, and the workspace arithmetic of both.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/rsvd_c.h"
#include "batched.hpp"
#include "handle.hpp"

using namespace rsvd;

namespace {

// The descriptor checks of rsvd_run (through rsvd_workspace_bytes, which needs no handle) plus the
// batch's own.  ldu / ldv = 0: not known (a workspace query): the outputs' smallest footprints count.
int check_batch(const rsvd_desc_t* d, const rsvd_batch_t* bt, int64_t ldu, int64_t ldv, const char** err) {
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
    if (bt->a_stride0 < 0 || bt->a_stride1 < 0 || bt->omega_stride < 0 || bt->u_stride < 0 || bt->s_stride < 0 ||
        bt->v_stride < 0) {
        *err = "negative batch stride";
        return RSVD_ERR_INVALID_ARG;
    }
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
    const char* err = "";
    if (ldu <= 0 || ldv <= 0) {
        h->err = "null pointer or bad leading dimension";
        return RSVD_ERR_INVALID_ARG;
    }
    const int st = check_batch(d, bt, ldu, ldv, &err);
    if (st != RSVD_OK) {
        h->err = err;
        return st;
    }
    if (h->world > 1) {
        h->err = "batched runs are single-GPU (the handle is row-sharded)";
        return RSVD_ERR_UNSUPPORTED;
    }
    if (!A || !U || !S || !V || (omega && ldo < d->n)) {
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
        RSVD_CK(launch_batched_rsvd(a, d->dtype, p.LP, p.plds, p.lds, p.grid, h->stream));
        return RSVD_OK;
    }
    // Outside the fused limits: rsvd_run per matrix on the same stream, seed + b.
    const size_t ib = in_bytes(d->dtype), ob = out_bytes(d->dtype);
    std::vector<int32_t> hinfo(info ? 2 * batch : 0);
    bool nonfinite = false;
    for (int64_t b = 0; b < batch; ++b) {
        const int64_t i0 = b % bt->count0, i1 = b / bt->count0;
        rsvd_desc_t db = *d;
        db.seed = d->seed + (uint64_t)b;
        const char* Ab = static_cast<const char*>(A) + ib * (size_t)(i0 * bt->a_stride0 + i1 * bt->a_stride1);
        const char* Ob = omega ? static_cast<const char*>(omega) + ob * (size_t)(b * bt->omega_stride) : nullptr;
        RSVD_TRY(rsvd_run(h, &db, Ab, Ob, ldo, static_cast<char*>(U) + ob * (size_t)(b * bt->u_stride), ldu,
                          static_cast<char*>(S) + ob * (size_t)(b * bt->s_stride),
                          static_cast<char*>(V) + ob * (size_t)(b * bt->v_stride), ldv));
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

}  // extern "C"
