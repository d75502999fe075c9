// wide_plan.cpp -- the planner of the bf16 / e4m3 projections (wide_proj.hip): which kernel a product
// runs on, its row blocks and its K split.  Host code only (no kernels), so a plain C++ compiler
// builds it and tests/cpp/plan_dump.cpp checks it without a GPU.
#include <cstdlib>

#include "wide.hpp"

namespace rsvd {

bool wproj_supported_lp(int LP) {
    return LP == 16 || LP == 32 || LP == 64 || LP == 128 || LP == 256 || LP == 512;
}

int wproj_rows_per_block(int LP) { return LP <= 128 ? 256 : (LP == 256 ? 128 : 64); }

const char* wproj_kernel_name(WProjKernel k) {
    switch (k) {
        case WProjKernel::Fallback: return "wproj";
        case WProjKernel::W2: return "wproj2";
        case WProjKernel::W2Ds: return "wproj2_ds";
        case WProjKernel::W2Half: return "wproj2_half";
        case WProjKernel::W3: return "wproj3";
        case WProjKernel::W3Tn2: return "wproj3tn2";
        case WProjKernel::W3Tn128: return "wproj3tn128";
        case WProjKernel::W3Tn4: return "wproj3tn4";
        case WProjKernel::W3Nn8: return "wproj3nn8";
    }
    return "?";
}

// A/B switches of the environment, read once per process (default 1: the newer kernel)
static bool env_switch(const char* name) {
    const char* v = std::getenv(name);
    return (v ? std::atoi(v) : 1) != 0;
}
static bool tn128_enabled() {  // RSVD_TN128=0: the W2Ds LP = 128 TN instead of W3Tn128
    static const bool on = env_switch("RSVD_TN128");
    return on;
}
static bool nn8_enabled() {  // RSVD_NN8=0: the W2Half e4m3 NN instead of W3Nn8
    static const bool on = env_switch("RSVD_NN8");
    return on;
}
static bool nn3_128_enabled() {  // RSVD_NN3_128=0: the W2 bf16 NN at LP = 128 instead of W3
    static const bool on = env_switch("RSVD_NN3_128");
    return on;
}

static WProjKernel choose_kernel(int64_t K, int LP, bool v2, bool nn, bool fp8) {
    typedef WProjKernel W;
    if (!v2 || LP < 128) return W::Fallback;
    if (LP == 128) {
        if (fp8) return W::W2;
        if (nn) return nn3_128_enabled() ? W::W3 : W::W2;
        if (K % 64 != 0) return W::W2;  // the double-step stages need whole 64-row K chunks
        return tn128_enabled() ? W::W3Tn128 : W::W2Ds;
    }
    if (!fp8) return (!nn && LP == 256) ? W::W3Tn2 : W::W3;
    if (!nn) return W::W3Tn4;
    if (LP == 256) return W::W2;
    return nn8_enabled() ? W::W3Nn8 : W::W2Half;
}

WProjKernel wproj_kernel_for(const WProjPlan& p, bool split) {
    // the v3 NN at LP = 128 (WI = 512 rows, A 3 / S 2 slots) for the hi / lo products: C3 5.40 ->
    // 5.35 ms (gpurun_out r6d, bit-identical); the single-pass sketch measured 468 -> 473 us on it
    // and keeps v2 (same 512-row blocks, so one plan serves both)
    if (p.kernel == WProjKernel::W3 && p.LP == 128 && !split) return WProjKernel::W2;
    return p.kernel;
}

bool wproj_plan_valid(const WProjPlan& p) {
    const bool wide = p.LP == 256 || p.LP == 512;
    switch (p.kernel) {
        case WProjKernel::Fallback: return wproj_supported_lp(p.LP);
        case WProjKernel::W2: return p.LP == 128 || (p.LP == 256 && p.fp8 && p.nn);
        case WProjKernel::W2Ds:
        case WProjKernel::W3Tn128: return p.LP == 128 && !p.fp8 && !p.nn;
        case WProjKernel::W2Half:
        case WProjKernel::W3Nn8: return p.LP == 512 && p.fp8 && p.nn;
        case WProjKernel::W3: return !p.fp8 && (wide || (p.LP == 128 && p.nn));
        case WProjKernel::W3Tn2: return p.LP == 256 && !p.fp8 && !p.nn;
        case WProjKernel::W3Tn4: return wide && p.fp8 && !p.nn;
    }
    return false;
}

// output rows per workgroup
static int rows_per_block(WProjKernel k, int LP) {
    switch (k) {
        case WProjKernel::Fallback: return wproj_rows_per_block(LP);
        case WProjKernel::W2:
        case WProjKernel::W3: return 65536 / LP;  // 512 / 256 / 128 rows at LP 128 / 256 / 512
        default: return 256;
    }
}

// K quantum of a chunk: whole A slots / stages of the kernel
static int chunk_quantum(WProjKernel k) {
    switch (k) {
        case WProjKernel::W3Tn4: return 4 * kWprojKStep;  // four k-steps per A slot: whole 128-row slots
        case WProjKernel::W2Ds:
        case WProjKernel::W3Tn128:
        case WProjKernel::W3Tn2: return 2 * kWprojKStep;  // two k-steps per stage / A slot: whole 64-row pairs
        default: return kWprojKStep;
    }
}

WProjPlan plan_wproj(int64_t rows_out, int64_t K, int LP, bool v2, bool nn, bool fp8) {
    typedef WProjKernel W;
    WProjPlan p;
    p.nn = nn;
    p.fp8 = fp8;
    p.LP = LP;
    p.kernel = choose_kernel(K, LP, v2, nn, fp8);
    const int WI = rows_per_block(p.kernel, LP);
    p.blocks = (int)((rows_out + WI - 1) / WI);
    // LP = 512 e4m3 products as two 256-column halves in one launch (twin workgroups adjacent)
    p.merge = LP == 512 && (p.kernel == W::W2Half || p.kernel == W::W3Nn8 || p.kernel == W::W3Tn4);
    // one workgroup per CU (LDS ring / registers); merged halves: two workgroups per (row block, split)
    const int target = p.merge ? 128 : ((p.kernel != W::Fallback || LP >= 512) ? 256 : 512);
    int64_t splits = (target + p.blocks - 1) / p.blocks;
    const int64_t max_by_work = K / (kWprojKStep * 8);
    if (splits > max_by_work) splits = max_by_work;
    if (splits > 128) splits = 128;
    if (splits < 1) splits = 1;
    int64_t chunk = (K + splits - 1) / splits;
    const int kq = chunk_quantum(p.kernel);
    chunk = (chunk + kq - 1) / kq * kq;
    p.chunk = chunk;
    p.splits = (int)((K + chunk - 1) / chunk);
    // the block-scaled K = 128 form of the e4m3 sketch when every stage is whole (else the K = 32 form)
    p.s8_scaled = wproj_s8_supported(p) && K % 128 == 0 && p.chunk % 128 == 0;
    return p;
}

bool wproj_s8_supported(const WProjPlan& p) {
    return p.nn && p.fp8 && p.kernel != WProjKernel::Fallback && (p.LP == 256 || p.LP == 512);
}

}  // namespace rsvd
