// wide_dev.hpp -- the device helpers more than one of wide_gram.hip, wide_chol.hip and wide_panel.hip uses.
#pragma once
#include "common.hpp"
#include "wide.hpp"

namespace rsvd {

typedef Mfma<double> MD;

typedef __attribute__((ext_vector_type(8))) short bf16x8s;  // one lane's A / B fragment of v_mfma_f32_16x16x32_bf16

// two fp32 -> packed bf16 (round to nearest even): lo = a, hi = b
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {
    uint32_t r;
    asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

__device__ __forceinline__ bf16_t f2bf(float x) {  // round to nearest even
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7f800000u) == 0x7f800000u) return (bf16_t)(u >> 16);
    return (bf16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf2f(bf16_t b) { return __uint_as_float((uint32_t)b << 16); }

// The three bf16 pieces of the fp32 element (row k, column c) of an LP x LP matrix in split_mat_kernel's
// transposed piece images (Mt[x][c][k], image pitch L2 = LP^2): the factor kernels that write R^-1's
// fp32 copy also write its pieces, so the split panel product needs no split_mat launch.
__device__ __forceinline__ void store_pieces(bf16_t* __restrict__ Mt, int64_t L2, int64_t idx, float v) {
    const bf16_t bh = f2bf(v);
    const float rm = v - bf2f(bh);
    const bf16_t bm = f2bf(rm);
    Mt[idx] = bh;
    Mt[L2 + idx] = bm;
    Mt[2 * L2 + idx] = f2bf(rm - bf2f(bm));
}

}  // namespace rsvd
