// Element-wise launches over n fp32 elements (air_concrete.hip, the stand-alone VAE gradients of air_pointwise.hip): a
// grid-stride loop whose body takes four elements per thread through 16-byte loads and stores when every array of the
// call is 16-byte aligned, and a scalar tail (all of it when something is not).  An op is a struct of pointers with
//   template <int W> __device__ void run(long i) const      -- elements i .. i + W - 1, W = 4 or 1
// built from ew_ld / ew_st / ew_lds below.
#pragma once
#include "air_common.h"

namespace {

constexpr int EW_THREADS = 256;

// air_scalar_t as the kernels take it
struct EwScalar { const float* p; float v; int stride; };

template <int W>
__device__ __forceinline__ void ew_ld(const float* __restrict__ p, long i, float (&v)[W]) {
    if constexpr (W == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[i];
    }
}
// a nullable array: zeros when absent
template <int W>
__device__ __forceinline__ void ew_ld0(const float* __restrict__ p, long i, float (&v)[W]) {
    if (p) ew_ld<W>(p, i, v);
    else {
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = 0.0f;
    }
}
template <int W>
__device__ __forceinline__ void ew_st(float* __restrict__ p, long i, const float (&v)[W]) {
    if constexpr (W == 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    else p[i] = v[0];
}
template <int W>
__device__ __forceinline__ void ew_lds(const EwScalar& s, long i, float (&v)[W]) {
    if (s.p && s.stride) ew_ld<W>(s.p, i, v);
    else {
        const float x = s.p ? s.p[0] : s.v;
#pragma unroll
        for (int k = 0; k < W; ++k) v[k] = x;
    }
}

template <class Op>
__global__ __launch_bounds__(EW_THREADS) void ew_kernel(Op op, long n, int vec) {
    const long tid = (long)blockIdx.x * EW_THREADS + threadIdx.x, nth = (long)gridDim.x * EW_THREADS;
    const long n4 = vec ? n / 4 : 0;
    for (long q = tid; q < n4; q += nth) op.template run<4>(q * 4);
    for (long i = n4 * 4 + tid; i < n; i += nth) op.template run<1>(i);
}

inline bool ew_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }     // (a null pointer counts as aligned)
inline bool ew_al16(const air_scalar_t& s) { return !(s.ptr && s.stride) || ew_al16(s.ptr); }
// null descriptor, or a stride that is neither "one value" nor "one per element"
inline bool ew_bad(const air_scalar_t* s) { return !s || (s->stride != 0 && s->stride != 1); }
inline EwScalar ew_scalar(const air_scalar_t& s) { return EwScalar{s.ptr, s.value, s.stride}; }

template <class Op>
int ew_launch(const Op& op, int64_t n, bool vec, void* stream) {
    const long work = vec ? (long)(n / 4 + n % 4) : (long)n;
    long blocks = (work + EW_THREADS - 1) / EW_THREADS;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(ew_kernel<Op>, dim3((int)blocks), dim3(EW_THREADS), 0, air_stream(stream), op, (long)n, vec ? 1 : 0);
    AIR_CHECK_LAUNCH();
    return 0;
}

}  // namespace
