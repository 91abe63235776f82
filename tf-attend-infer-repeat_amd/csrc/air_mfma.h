// What the GEMM kernels (air_gemm_common.h, namespace airg), the weight-gradient tiles (air_wgrad.hip, namespace airw) and
// the bottleneck kernels (air_bottleneck.hip) need and none of them owns: the MFMA operand / accumulator vector types,
// accumulator zeroing, gfx950's transpose read and the pointer-alignment predicates.  They import the names with
// using-declarations.
#pragma once
#include "air_common.h"

namespace airm {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

__host__ __device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
__host__ __device__ __forceinline__ bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

template <int TM, int TN>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[TM][TN]) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// gfx950 transpose read ds_read_b64_tr_b16, twice: from a [k][BN] bf16 image, lane i of a 16-lane group hands in the
// address of row 8g + i/4 (+4), column quad i%4 of the [k][16] block (blk); it receives k = 8g .. 8g+3 (+4) of
// column i -- the 8 consecutive k v_mfma_f32_16x16x32_bf16 wants
__device__ __forceinline__ bf16x8 read_tr_bf16x8(const unsigned short* blk, int BN) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(blk));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(blk + 4 * BN));
    return bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
}

}  // namespace airm
