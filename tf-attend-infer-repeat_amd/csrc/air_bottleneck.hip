// The VAE bottleneck as ONE launch per direction (vae.py:16-34).
//
// Forward:  ml = X.Wml + b (mean | log-variance), z = mean + eps*sqrt(exp(lv)), g = softplus(z.Wg + bg)
// Backward: d_z = dG.Wg^T, (d_mean | d_lv) from the reparameterisation + KL terms, d_x = (d_ml.Wml^T) * softplus'(x)
//
// As two GEMM launches each, these are the most latency-bound links of the chain (100 and 50 output
// columns: 4-48 workgroups that still pay a launch and a memory round trip each).  Here a workgroup owns
// 16 rows and a 64-column slice of the second product (blockIdx.y: columns of g forward, of d_x backward);
// the 2Z-wide first product is recomputed by each of the slices (it is tiny), stays in registers, goes
// through the reparameterisation in the MFMA accumulator layout and is handed to the second product through
// LDS -- no global round trip, no second launch.  Wave w owns the units 16w .. 16w+15 of the first product
// and the columns 16w .. 16w+15 of the slice.  The first product's results (ml, z, z16 forward; d_ml,
// d_ml16 backward) are stored by the slice-0 workgroups only; every slice stores its own columns of g / g16
// or d_x / d_x16.  Every global load of the workgroup is issued before the first is consumed: each staging
// part below has an issue half and a store half, and a kernel calls all issue halves, then the
// epilogue-operand loads, then the store halves, then the barrier.
//
// Six kernels, three operand forms:
//   bottleneck_{fwd,bwd}_kernel<256, false>  fp32 operands, rounded to bf16 on their way into the LDS images
//   bottleneck_{fwd,bwd}_kernel<256, true>   the operands' bf16 twins (the producing GEMM's C16 / Adam's shadow), copied
//                                            into the same images: half the bytes, no conversion, the same bits
//   bottleneck_{fwd,bwd}_f32_kernel<256>     exact fp32 (air_bottleneck_*_t.exact_fp32): fp32 images, products on
//                                            v_mfma_f32_16x16x4_f32.  No model path uses them (air_model.py: the fp32 model
//                                            runs two air_gemm launches instead); they are kept for the graph-golden test.
//
// bf16 operand images in LDS are [row or column][k] with a row stride of K + 8 elements: consecutive rows
// shift by 16 bytes, so the 16-lane ds_read_b128 fragment groups are bank-conflict free without a swizzle.
#include "air_mfma.h"
#include <type_traits>

namespace {

using airm::f32x4;
using airm::bf16x8;
using airm::aligned16;
using airm::aligned8;
constexpr int THREADS = 256;
constexpr int PAD = 8;                             // bf16 elements
constexpr int FPAD = 4;                            // floats: 16-byte row shift of the k-contiguous fp32 images

// 16-byte load of a row-major operand with the out-of-range case redirected to element 0 (branch-free;
// the caller zeroes what was out of range when it consumes the value)
__device__ __forceinline__ float4 fetch16(const float* __restrict__ base, bool ok, size_t at) {
    return *reinterpret_cast<const float4*>(base + (ok ? at : 0));
}
__device__ __forceinline__ float4 zero_unless(bool ok, float4 v) {
    return ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float comp(const float4& t, int j) { return j == 0 ? t.x : j == 1 ? t.y : j == 2 ? t.z : t.w; }

// twin operands: 8 / 16 bytes of bf16 with the out-of-range case redirected to element 0 and zeroed by a bit mask
__device__ __forceinline__ uint2 fetch8(const unsigned short* __restrict__ base, bool ok, size_t at) {
    const uint2 t = *reinterpret_cast<const uint2*>(base + (ok ? at : 0));
    const unsigned m = ok ? 0xffffffffu : 0u;
    return make_uint2(t.x & m, t.y & m);
}
__device__ __forceinline__ uint4 fetch16(const unsigned short* __restrict__ base, bool ok, size_t at) {
    const uint4 t = *reinterpret_cast<const uint4*>(base + (ok ? at : 0));
    const unsigned m = ok ? 0xffffffffu : 0u;
    return make_uint4(t.x & m, t.y & m, t.z & m, t.w & m);
}
// four consecutive elements of either kind
__device__ __forceinline__ float4 fetch_quad(const float* __restrict__ base, bool ok, size_t at) { return fetch16(base, ok, at); }
__device__ __forceinline__ uint2 fetch_quad(const unsigned short* __restrict__ base, bool ok, size_t at) { return fetch8(base, ok, at); }
// element j (0..3) of the four bf16 a row piece holds, from two rows -> one dword of a [column][k] image
__device__ __forceinline__ unsigned pair16(const uint2& r0, const uint2& r1, int j) {
    const unsigned a = j < 2 ? r0.x : r0.y, b = j < 2 ? r1.x : r1.y;
    return (j & 1) ? ((a >> 16) | (b & 0xffff0000u)) : ((a & 0xffffu) | (b << 16));
}

// A register piece into an image, one overload per operand form: fp32 -> bf16 pack, bf16 twin copy, fp32 copy.
// `ok` zeroes the fp32 pieces that were fetched out of range; a twin piece was masked when it was fetched.
__device__ __forceinline__ void put(unsigned short* at, const float4& v, bool ok) {
    const float4 x = zero_unless(ok, v);
    uint2 w; w.x = air_pack_bf16(x.x, x.y); w.y = air_pack_bf16(x.z, x.w);
    *reinterpret_cast<uint2*>(at) = w;
}
__device__ __forceinline__ void put(unsigned short* at, const uint4& v, bool) { *reinterpret_cast<uint4*>(at) = v; }
__device__ __forceinline__ void put(unsigned short* at, const uint2& v, bool) { *reinterpret_cast<uint2*>(at) = v; }
__device__ __forceinline__ void put(float* at, const float4& v, bool ok) { *reinterpret_cast<float4*>(at) = zero_unless(ok, v); }

// the operand a kernel instance reads: the fp32 array or its bf16 twin
template <bool TW> __device__ __forceinline__ auto twin_or(const float* f, const unsigned short* h) {
    if constexpr (TW) return h; else return f;
}

// ROWS x K of a row-major operand, k contiguous, in 16-byte pieces (4 floats / 8 bf16), consecutive lanes along the
// row: X of the forward, dG and Wg of the backward.  E = float or unsigned short (twin); the image's element type picks
// pack or copy.  Row `row` of the tile is row row0 + row of the operand and is live while row0 + row < lim.
template <typename E, int ROWS, int K>
struct RowTile {
    static constexpr int W = 16 / sizeof(E), N = ROWS * K / W / THREADS;
    std::conditional_t<std::is_same_v<E, float>, float4, uint4> r[N];
    __device__ __forceinline__ void issue(const E* __restrict__ base, int ld, int row0, int lim, int tid) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int t = tid + THREADS * i, row = t / (K / W), c = t % (K / W);
            r[i] = fetch16(base, row0 + row < lim, (size_t)(row0 + row) * ld + c * W);
        }
    }
    template <typename I>
    __device__ __forceinline__ void store(I* img, int L, int row0, int lim, int tid) const {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int t = tid + THREADS * i, row = t / (K / W), c = t % (K / W);
            put(&img[row * L + c * W], r[i], row0 + row < lim);
        }
    }
};

// Rows j0 .. j0+63 of Wml [K1, 2Z] for the backward's second product, k = 2Z contiguous, in quads (2Z % 4 == 0: Z is
// even), densely packed over the threads: t -> (row t / NQ, quad t % NQ), 64 rows x <= 32 quads / 256 threads
template <typename E>
struct WmlSlice {
    static constexpr int NM = 8;
    std::conditional_t<std::is_same_v<E, float>, float4, uint2> r[NM];
    int nq;                                        // quads per row, <= 32
    unsigned inv_nq;                               // t / nq == (t * inv_nq) >> 20 for t < 2048, nq <= 32
    __device__ __forceinline__ void issue(const E* __restrict__ Wml, int j0, int K1, int Z2, int tid) {
        nq = (Z2 + 3) >> 2;
        inv_nq = ((1u << 20) + nq - 1) / nq;
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int t = tid + THREADS * i;
            const int row = (int)(((unsigned)t * inv_nq) >> 20), c4 = t - row * nq;
            r[i] = fetch_quad(Wml, row < 64 && j0 + row < K1, (size_t)(j0 + row) * Z2 + c4 * 4);
        }
    }
    template <typename I>
    __device__ __forceinline__ void store(I* B2, int L2, int j0, int K1, int tid) const {
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int t = tid + THREADS * i;
            const int row = (int)(((unsigned)t * inv_nq) >> 20), c4 = t - row * nq;
            if (row >= 64) continue;
            put(&B2[row * L2 + c4 * 4], r[i], j0 + row < K1);
        }
    }
};

// zero `bytes` (a multiple of 16) of LDS
__device__ __forceinline__ void zero_lds(void* p, int bytes, int tid) {
    for (int i = tid; i < bytes / 16; i += THREADS) reinterpret_cast<uint4*>(p)[i] = make_uint4(0u, 0u, 0u, 0u);
}

// a value as an element of the second product's A image: bf16 (RNE) or fp32
template <typename T> __device__ __forceinline__ T image_of(float v) {
    if constexpr (std::is_same_v<T, float>) return v; else return air_bf16_of(v);
}

// fragment of a [row][k] bf16 image: lane l -> row (l & 15), the 8 k of slot ks*4 + (l >> 4)
__device__ __forceinline__ bf16x8 frag(const unsigned short* img, int ld, int row0, int ks, int lane) {
    return *reinterpret_cast<const bf16x8*>(&img[(row0 + (lane & 15)) * ld + ks * 32 + (lane >> 4) * 8]);
}

// Exact-fp32 products on v_mfma_f32_16x16x4_f32.  One 16-byte LDS read of a k-contiguous operand feeds FOUR MFMAs through
// the k-permutation gemm_f32v2_kernel uses: lane l supplies k = 16 kb + 4 (l >> 4) + e to the e-th of them, for A and B
// alike.  A [16][lda] is k-contiguous in both forms.
// kk: B [..][ldb] k-contiguous too, this lane's column is row `brow` of it
template <int UNROLL>
__device__ __forceinline__ void mfma_f32_kk(f32x4& acc, const float* A, int lda, const float* B, int ldb, int brow, int nkb, int lane) {
#pragma unroll UNROLL
    for (int kb = 0; kb < nkb; ++kb) {
        const int k0 = kb * 16 + (lane >> 4) * 4;
        const float4 av = *reinterpret_cast<const float4*>(&A[(lane & 15) * lda + k0]);
        const float4 bv = *reinterpret_cast<const float4*>(&B[brow * ldb + k0]);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bv.w, acc, 0, 0, 0);
    }
}
// kn: B [k][ldb] is a row-major [K, N] weight AS IT LIES (coalesced copies into LDS), its fragments read as four scalars
// per 16 k -- a register transposition into [column][k] images would cost these latency-bound kernels more than the scalar
// reads do.  One A read feeds NACC accumulators, accumulator j from column col[j] of B.
template <int UNROLL, int NACC>
__device__ __forceinline__ void mfma_f32_kn(f32x4 (&acc)[NACC], const float* A, int lda, const float* B, int ldb, const int (&col)[NACC],
                                            int nkb, int lane) {
#pragma unroll UNROLL
    for (int kb = 0; kb < nkb; ++kb) {
        const int k0 = kb * 16 + (lane >> 4) * 4;
        const float4 av = *reinterpret_cast<const float4*>(&A[(lane & 15) * lda + k0]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ae = comp(av, e);
#pragma unroll
            for (int j = 0; j < NACC; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ae, B[(k0 + e) * ldb + col[j]], acc[j], 0, 0, 0);
        }
    }
}

// ---- forward: epilogue operands, reparameterisation, output store -----------------------------------------------------
// NONNEG: the entry points admit only M, Z, K1 > 0, and the epilogue loads say so to the compiler.  The signed 64-bit row
// offset (size_t)m * Z then is one unsigned multiply-add; as a signed product it expands into two, the second with an
// undefined high half as its addend, and the register allocator is free to overlap that half with the destination of a
// load still in flight -- an s_waitcnt vmcnt(0) in the middle of the load phase.
// in the accumulator layout: row = (lane>>4)*4 + q, unit / column = 16*wave + (lane&15)
struct FwdEpi {
    float e_eps[4], b_mean, b_lv, b_g;
    int u, n;                                      // unit of the first product, column of g
};
__device__ __forceinline__ FwdEpi fwd_epi_load(const air_bottleneck_fwd_t& a, int m0, int n0, int lane, int wave) {
    FwdEpi e;
    e.u = wave * 16 + (lane & 15);
    const bool uok = e.u < a.Z;
    __builtin_assume(a.Z > 0);                     // (NONNEG below)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = m0 + (lane >> 4) * 4 + q;
        __builtin_assume(m >= 0);
        e.e_eps[q] = a.eps[(uok && m < a.M) ? (size_t)m * a.Z + e.u : 0];
    }
    e.b_mean = a.bml[uok ? e.u : 0];
    e.b_lv = a.bml[uok ? a.Z + e.u : 0];
    e.n = n0 + e.u;
    e.b_g = a.bg[e.n < a.H ? e.n : 0];
    return e;
}

// vae.py:16-24: mean | log_var (+bias), sample = mean + eps*sqrt(exp(lv)); the slice-0 workgroups store them (and z16
// where A2 is a bf16 image); every workgroup hands z to the second product in A2 [16][L2], zero beyond unit Z and row M
template <typename T>
__device__ __forceinline__ void reparam(const air_bottleneck_fwd_t& a, const FwdEpi& e, const f32x4& am, const f32x4& al, T* A2, int L2,
                                        int m0, int lane) {
    const int M = a.M, Z = a.Z, Z2 = 2 * a.Z, u = e.u;
    const bool uok = u < Z;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = (lane >> 4) * 4 + q, m = m0 + row;
        const float mean = am[q] + e.b_mean, lv = al[q] + e.b_lv;
        const float zz = mean + e.e_eps[q] * sqrtf(expf(lv));
        if (blockIdx.y == 0 && uok && m < M) {
            a.ml[(size_t)m * Z2 + u] = mean;
            a.ml[(size_t)m * Z2 + Z + u] = lv;
            a.z[(size_t)m * a.ldz + u] = zz;
            if constexpr (std::is_same_v<T, unsigned short>)
                if (a.z16) a.z16[(size_t)m * a.ldz + u] = air_bf16_of(zz);
        }
        A2[row * L2 + u] = (uok && m < M) ? image_of<T>(zz) : T(0);
    }
}

// g = softplus(z.Wg + bg), the columns of this slice; g16 nullable
__device__ __forceinline__ void store_g(const air_bottleneck_fwd_t& a, const FwdEpi& e, const f32x4& ag, unsigned short* g16, int m0, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = m0 + (lane >> 4) * 4 + q;
        if (m < a.M && e.n < a.H) {
            const float gv = air_softplus(ag[q] + e.b_g);
            a.g[(size_t)m * a.H + e.n] = gv;
            if (g16) g16[(size_t)m * a.H + e.n] = air_bf16_of(gv);
        }
    }
}

// ---- backward: epilogue operands, KL + reparameterisation gradient, output store -----------------------------------------
struct BwdEpi {
    float e_mean[4], e_lv[4], e_eps[4], e_mask[4], e_x[4], gs, pv, pm;
    int u, jn;                                     // unit of the first product, column of d_x
};
__device__ __forceinline__ BwdEpi bwd_epi_load(const air_bottleneck_bwd_t& a, int m0, int j0, int lane, int wave) {
    BwdEpi e;
    const int M = a.M, Z = a.Z, Z2 = 2 * a.Z, K1 = a.K1;
    e.u = wave * 16 + (lane & 15);
    const bool uok = e.u < Z;
    e.jn = j0 + e.u;
    __builtin_assume(Z > 0); __builtin_assume(K1 > 0);   // (NONNEG)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = m0 + (lane >> 4) * 4 + q;
        __builtin_assume(m >= 0);
        const bool ok = uok && m < M;
        e.e_mean[q] = a.ml[ok ? (size_t)m * Z2 + e.u : 0];
        e.e_lv[q] = a.ml[ok ? (size_t)m * Z2 + Z + e.u : 0];
        e.e_eps[q] = a.eps[ok ? (size_t)m * Z + e.u : 0];
        e.e_mask[q] = a.att[m < M ? (size_t)m * AIR_ATT_STRIDE + AIR_ATT_MASK : 0];
        e.e_x[q] = a.x[(m < M && e.jn < K1) ? (size_t)m * K1 + e.jn : 0];
    }
    e.gs = a.dyn[AIR_DYN_GRAD_SCALE]; e.pv = a.dyn[AIR_DYN_VAE_PV]; e.pm = a.dyn[AIR_DYN_VAE_PM];
    return e;
}

// vae.py:22-24 + the KL of air_model.py:386-392: d loss / d mean, d loss / d log-variance; the slice-0 workgroups store
// them (and d_ml16 where A2 is a bf16 image); every workgroup hands them to the second product in A2 [16][L2], d_mean at
// u, d_lv at Z + u (the rest of A2 was zeroed)
template <typename T>
__device__ __forceinline__ void kl_reparam_grad(const air_bottleneck_bwd_t& a, const BwdEpi& e, const f32x4& az, T* A2, int L2, int m0,
                                                int lane) {
    const int M = a.M, Z = a.Z, Z2 = 2 * a.Z, u = e.u;
    const bool uok = u < Z;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int row = (lane >> 4) * 4 + q, m = m0 + row;
        const float klg = e.e_mask[q] * e.gs;
        const float var = expf(e.e_lv[q]);
        const float sd = sqrtf(var);
        const float d = az[q];
        const float dmean = d + klg * (e.e_mean[q] - e.pm) / e.pv;
        const float dlv = d * e.e_eps[q] * 0.5f * sd + klg * 0.5f * (var / e.pv - 1.0f);
        if (uok && m < M) {
            if (blockIdx.y == 0) {
                a.d_ml[(size_t)m * Z2 + u] = dmean; a.d_ml[(size_t)m * Z2 + Z + u] = dlv;
                if constexpr (std::is_same_v<T, unsigned short>)
                    if (a.d_ml16) { a.d_ml16[(size_t)m * Z2 + u] = air_bf16_of(dmean); a.d_ml16[(size_t)m * Z2 + Z + u] = air_bf16_of(dlv); }
            }
            A2[row * L2 + u] = image_of<T>(dmean);
            A2[row * L2 + Z + u] = image_of<T>(dlv);
        }
    }
}

// d_x = (d_ml . Wml^T) * softplus'(x), the columns of this slice; d_x16 nullable
__device__ __forceinline__ void store_dx(const air_bottleneck_bwd_t& a, const BwdEpi& e, const f32x4& ax, unsigned short* d_x16, int m0, int lane) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int m = m0 + (lane >> 4) * 4 + q;
        if (m < a.M && e.jn < a.K1) {
            const float dxv = ax[q] * (1.0f - expf(-e.e_x[q]));
            a.d_x[(size_t)m * a.K1 + e.jn] = dxv;
            if (d_x16) d_x16[(size_t)m * a.K1 + e.jn] = air_bf16_of(dxv);
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The kernels.  Their argument is the public struct (air_hip.h) with ldz resolved.
// ---------------------------------------------------------------------------------------------------------------------

// K1 = width of X (the last recognition layer), compile-time
// TW: X, Wml and Wg are read from their bf16 twins: half the bytes through the CU's vector-memory path (65 instead of
// 129 KB per workgroup), no conversion; the RNE twins are what air_pack_bf16 makes of the fp32 arrays, so both forms give
// the same bits.
template <int K1, bool TW>
__global__ __launch_bounds__(THREADS) void bottleneck_fwd_kernel(air_bottleneck_fwd_t a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    constexpr int L1 = K1 + PAD, L2 = 64 + PAD;
    unsigned short* A1 = smem;                    // [16][L1]   X tile
    unsigned short* B1 = A1 + 16 * L1;            // [128][L1]  Wml columns: mean unit u at u, log-variance unit u at 64 + u
    unsigned short* A2 = B1 + 128 * L1;           // [16][L2]   z tile, k >= Z zero
    unsigned short* B2 = A2 + 16 * L2;            // [64][L2]   Wg columns of this slice, k >= Z zero

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 64;
    const int M = a.M, Z = a.Z, H = a.H, Z2 = 2 * a.Z;

    // ---- every load of the workgroup, back to back ------------------------------------------------
    RowTile<std::conditional_t<TW, unsigned short, float>, 16, K1> x;
    x.issue(twin_or<TW>(a.X, a.X16), a.ldx, m0, M, tid);
    // Wml [K1, 2Z] (columns contiguous): task = (k-run g of 8 rows, column quad) -> 8 quads, transposed in registers
    const int NQ = (Z2 + 3) >> 2;
    const int ntask = NQ * (K1 / 8);
    constexpr int NW = 4;                          // tasks per thread: 2Z <= 128 -> <= 32 quads x K1/8 runs <= 1024 (K1 = 256)
    float4 vw[TW ? 1 : NW][8];
    uint2 vwh[TW ? NW : 1][8];
    int wg_[NW], wq_[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int t = tid + THREADS * i;
        const bool ok = t < ntask;
        const int g = ok ? t / NQ : 0, cq = ok ? t - g * NQ : 0;
        wg_[i] = ok ? g : -1; wq_[i] = cq;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (TW) vwh[i][r] = fetch8(a.Wml16, ok, (size_t)(g * 8 + r) * Z2 + cq * 4);
            else vw[i][r] = fetch16(a.Wml, ok, (size_t)(g * 8 + r) * Z2 + cq * 4);
        }
    }
    // Wg [Z, H] slice (columns n0 .. n0+63 contiguous): threads 0..127, task = (k-run g, column quad)
    float4 vg[TW ? 1 : 8];
    uint2 vgh[TW ? 8 : 1];
    const int gg = (tid >> 4) & 7, gq = tid & 15;
    const bool gcol = tid < 128 && n0 + gq * 4 < H;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        if (TW) vgh[r] = fetch8(a.Wg16, gcol && gg * 8 + r < Z, (size_t)(gg * 8 + r) * H + n0 + gq * 4);
        else vg[r] = fetch16(a.Wg, gcol && gg * 8 + r < Z, (size_t)(gg * 8 + r) * H + n0 + gq * 4);
    }
    const FwdEpi e = fwd_epi_load(a, m0, n0, lane, wave);

    // ---- into the images (fp32 operands: rounded to bf16 here) -----------------------------------------
    x.store(A1, L1, m0, M, tid);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        if (wg_[i] < 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = wq_[i] * 4 + j;
            if (c >= Z2) continue;
            const int col = c < Z ? c : 64 + (c - Z);
            uint4 w;
            if (TW) {
                w = make_uint4(pair16(vwh[i][0], vwh[i][1], j), pair16(vwh[i][2], vwh[i][3], j),
                               pair16(vwh[i][4], vwh[i][5], j), pair16(vwh[i][6], vwh[i][7], j));
            } else {
                w.x = air_pack_bf16(comp(vw[i][0], j), comp(vw[i][1], j)); w.y = air_pack_bf16(comp(vw[i][2], j), comp(vw[i][3], j));
                w.z = air_pack_bf16(comp(vw[i][4], j), comp(vw[i][5], j)); w.w = air_pack_bf16(comp(vw[i][6], j), comp(vw[i][7], j));
            }
            *reinterpret_cast<uint4*>(&B1[col * L1 + wg_[i] * 8]) = w;
        }
    }
    if (tid < 128) {
        float4 t8[8];
        if (!TW) {
#pragma unroll
            for (int r = 0; r < 8; ++r) t8[r] = zero_unless(gcol && gg * 8 + r < Z, vg[r]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint4 w;
            if (TW) {
                w = make_uint4(pair16(vgh[0], vgh[1], j), pair16(vgh[2], vgh[3], j), pair16(vgh[4], vgh[5], j), pair16(vgh[6], vgh[7], j));
            } else {
                w.x = air_pack_bf16(comp(t8[0], j), comp(t8[1], j)); w.y = air_pack_bf16(comp(t8[2], j), comp(t8[3], j));
                w.z = air_pack_bf16(comp(t8[4], j), comp(t8[5], j)); w.w = air_pack_bf16(comp(t8[6], j), comp(t8[7], j));
            }
            *reinterpret_cast<uint4*>(&B2[(gq * 4 + j) * L2 + gg * 8]) = w;
        }
    }
    __syncthreads();

    // ---- first product: wave w owns the units 16w .. 16w+15, mean and log-variance in the same lanes --
    f32x4 am = {0.f, 0.f, 0.f, 0.f}, al = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < K1 / 32; ++ks) {
        const bf16x8 av = frag(A1, L1, 0, ks, lane);
        am = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, frag(B1, L1, wave * 16, ks, lane), am, 0, 0, 0);
        al = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, frag(B1, L1, 64 + wave * 16, ks, lane), al, 0, 0, 0);
    }
    reparam(a, e, am, al, A2, L2, m0, lane);
    __syncthreads();

    // ---- second product: wave w owns columns n0 + 16w .. of this slice -------------------------------
    f32x4 ag = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
        ag = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(A2, L2, 0, ks, lane), frag(B2, L2, wave * 16, ks, lane), ag, 0, 0, 0);
    store_g(a, e, ag, a.g16, m0, lane);
}

// H = width of dG (the first generative layer), compile-time
// TW: dG, Wg and Wml from their bf16 twins -- all three are k-contiguous here, i.e. straight 16 / 8-byte copies into the
// images (46 instead of 93 KB per workgroup through the vector-memory path, no conversion)
template <int H, bool TW>
__global__ __launch_bounds__(THREADS) void bottleneck_bwd_kernel(air_bottleneck_bwd_t a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    constexpr int L1 = H + PAD, L2 = 128 + PAD;
    unsigned short* A1 = smem;                    // [16][L1]   dG tile
    unsigned short* B1 = A1 + 16 * L1;            // [64][L1]   Wg rows (unit z; rows >= Z unused)
    unsigned short* A2 = B1 + 64 * L1;            // [16][L2]   d_ml tile (d_mean at u, d_lv at Z + u), k >= 2Z zero
    unsigned short* B2 = A2 + 16 * L2;            // [64][L2]   Wml rows of this slice, k >= 2Z zero

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * 16, j0 = blockIdx.y * 64;
    using E = std::conditional_t<TW, unsigned short, float>;

    // ---- every load, back to back ---------------------------------------------------------------------
    RowTile<E, 16, H> dg;
    dg.issue(twin_or<TW>(a.dG, a.dG16), H, m0, a.M, tid);
    RowTile<E, 64, H> wg;                         // Wg [Z, H]: row z is k-contiguous already; rows >= Z are not loaded
    wg.issue(twin_or<TW>(a.Wg, a.Wg16), H, 0, a.Z, tid);
    WmlSlice<E> wm;
    wm.issue(twin_or<TW>(a.Wml, a.Wml16), j0, a.K1, 2 * a.Z, tid);
    const BwdEpi e = bwd_epi_load(a, m0, j0, lane, wave);

    // zero the second product's images: their k padding (>= 2Z) must not meet stale LDS contents
    zero_lds(A2, (16 + 64) * L2 * (int)sizeof(unsigned short), tid);

    // ---- into the images (fp32 operands: rounded to bf16 here) --------------------------------------------
    dg.store(A1, L1, m0, a.M, tid);
    wg.store(B1, L1, 0, a.Z, tid);
    __syncthreads();                               // the zero fill is complete before anything lands in A2 / B2
    wm.store(B2, L2, j0, a.K1, tid);

    // ---- first product: d_z for the units of this wave ----------------------------------------------------
    f32x4 az = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < H / 32; ++ks)
        az = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(A1, L1, 0, ks, lane), frag(B1, L1, wave * 16, ks, lane), az, 0, 0, 0);
    kl_reparam_grad(a, e, az, A2, L2, m0, lane);
    __syncthreads();

    // ---- second product: d_x = (d_ml . Wml^T) * softplus'(x), columns j0 + 16w .. -----------------------------
    f32x4 ax = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
        ax = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag(A2, L2, 0, ks, lane), frag(B2, L2, wave * 16, ks, lane), ax, 0, 0, 0);
    store_dx(a, e, ax, a.d_x16, m0, lane);
}

// ---- EXACT-fp32 forms: the same work split and hand-over through LDS; operands stay fp32 (mfma_f32_kk / mfma_f32_kn).
// Limits: K1 = 256 / H = 256; forward 2 Z <= 104.  Twins are neither read nor written.
template <int K1>
__global__ __launch_bounds__(THREADS) void bottleneck_fwd_f32_kernel(air_bottleneck_fwd_t a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    constexpr int L1 = K1 + FPAD, LW = 104 + FPAD, L2 = 64 + FPAD;
    float* A1 = reinterpret_cast<float*>(smem);   // [16][L1]   X tile, k contiguous
    float* B1 = A1 + 16 * L1;                     // [K1][LW]   Wml as it lies: column c < 2Z of row k at k * LW + c
    float* A2 = B1 + K1 * LW;                     // [16][L2]   z tile, k (unit) contiguous, k >= Z zero
    float* B2 = A2 + 16 * L2;                     // [64][L2]   Wg rows k < Z of this slice as they lie, rows >= Z zero

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * 16, n0 = blockIdx.y * 64;
    const int M = a.M, Z = a.Z, H = a.H, Z2 = 2 * a.Z;

    // ---- every load of the workgroup, back to back ------------------------------------------------
    RowTile<float, 16, K1> x;
    x.issue(a.X, a.ldx, m0, M, tid);
    const int NQ = Z2 >> 2;                        // float4 per row of Wml (Z even: whole quads), <= 26
    const int ntask = NQ * K1;
    constexpr int NW = (26 * K1 + THREADS - 1) / THREADS;
    float4 vw[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int t = tid + THREADS * i;
        vw[i] = fetch16(a.Wml, t < ntask, (size_t)t * 4);                  // (rows are contiguous: task t = quad t of the matrix)
    }
    constexpr int NGQ = 64 * 16 / THREADS;         // Wg slice: 64 rows x 16 quads
    float4 vg[NGQ];
#pragma unroll
    for (int i = 0; i < NGQ; ++i) {
        const int t = tid + THREADS * i, row = t >> 4, c4 = t & 15;
        vg[i] = fetch16(a.Wg, row < Z && n0 + c4 * 4 < H, (size_t)row * H + n0 + c4 * 4);
    }
    const FwdEpi e = fwd_epi_load(a, m0, n0, lane, wave);

    // ---- into LDS -------------------------------------------------------------------------------------
    x.store(A1, L1, m0, M, tid);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int t = tid + THREADS * i;
        if (t < ntask) {
            const int row = t / NQ, c4 = t - row * NQ;
            *reinterpret_cast<float4*>(&B1[row * LW + c4 * 4]) = vw[i];
        }
    }
#pragma unroll
    for (int i = 0; i < NGQ; ++i) {
        const int t = tid + THREADS * i, row = t >> 4, c4 = t & 15;
        put(&B2[row * L2 + c4 * 4], vg[i], row < Z && n0 + c4 * 4 < H);
    }
    __syncthreads();

    // ---- first product: wave w owns the units 16w .. 16w+15, mean and log-variance in the same lanes --
    // (units >= Z read columns that belong to other units or lie in the row padding: finite or not, they only reach
    // output columns nobody stores; the index is clamped so that every read stays inside the image)
    f32x4 aml[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const int cml[2] = {min(e.u, LW - 1), min(Z + e.u, LW - 1)};
    mfma_f32_kn<4>(aml, A1, L1, B1, LW, cml, K1 / 16, lane);
    reparam(a, e, aml[0], aml[1], A2, L2, m0, lane);
    __syncthreads();

    // ---- second product: wave w owns columns n0 + 16w .. of this slice (K = 64 units, zero beyond Z) --
    f32x4 ag[1] = {{0.f, 0.f, 0.f, 0.f}};
    const int cg[1] = {e.u};
    mfma_f32_kn<4>(ag, A2, L2, B2, L2, cg, 4, lane);
    store_g(a, e, ag[0], nullptr, m0, lane);
}

template <int H>
__global__ __launch_bounds__(THREADS) void bottleneck_bwd_f32_kernel(air_bottleneck_bwd_t a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned short smem[];
    constexpr int L1 = H + FPAD, L2 = 128 + FPAD;
    float* A1 = reinterpret_cast<float*>(smem);   // [16][L1]   dG tile
    float* B1 = A1 + 16 * L1;                     // [64][L1]   Wg rows (unit z; rows >= Z zero)
    float* A2 = B1 + 64 * L1;                     // [16][L2]   d_ml tile (d_mean at u, d_lv at Z + u), k >= 2Z zero
    float* B2 = A2 + 16 * L2;                     // [64][L2]   Wml rows of this slice, k >= 2Z zero

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * 16, j0 = blockIdx.y * 64;

    RowTile<float, 16, H> dg;
    dg.issue(a.dG, H, m0, a.M, tid);
    RowTile<float, 64, H> wg;
    wg.issue(a.Wg, H, 0, a.Z, tid);
    WmlSlice<float> wm;
    wm.issue(a.Wml, j0, a.K1, 2 * a.Z, tid);
    const BwdEpi e = bwd_epi_load(a, m0, j0, lane, wave);

    // zero the second product's images: their k padding (>= 2Z) must not meet stale LDS contents
    zero_lds(A2, (16 + 64) * L2 * (int)sizeof(float), tid);
    dg.store(A1, L1, m0, a.M, tid);
    wg.store(B1, L1, 0, a.Z, tid);
    __syncthreads();                               // the zero fill is complete before anything lands in A2 / B2
    wm.store(B2, L2, j0, a.K1, tid);

    // ---- first product: d_z for the units of this wave (both operands k-contiguous) ------------------------
    f32x4 az = {0.f, 0.f, 0.f, 0.f};
    mfma_f32_kk<4>(az, A1, L1, B1, L1, e.u, H / 16, lane);
    kl_reparam_grad(a, e, az, A2, L2, m0, lane);
    __syncthreads();

    // ---- second product: d_x = (d_ml . Wml^T) * softplus'(x), columns j0 + 16w .. (K = 128, zero beyond 2Z) ----
    f32x4 ax = {0.f, 0.f, 0.f, 0.f};
    mfma_f32_kk<8>(ax, A2, L2, B2, L2, e.u, 8, lane);
    store_dx(a, e, ax, nullptr, m0, lane);
}

// grant the dynamic LDS, launch, check
template <typename Kern, typename Args>
int launch(Kern kernel, dim3 grid, size_t lds, void* stream, const Args& a) {
    const int rc = air_grant_lds(reinterpret_cast<const void*>(kernel), lds);
    if (rc) return rc;
    hipLaunchKernelGGL(kernel, grid, dim3(THREADS), lds, air_stream(stream), a);
    AIR_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" int air_vae_bottleneck_fwd(const air_bottleneck_fwd_t* a, void* stream) {
    if (!a || !a->X || !a->Wml || !a->bml || !a->eps || !a->Wg || !a->bg || !a->ml || !a->z || !a->g) return AIR_EINVAL;
    if (a->M <= 0 || a->K1 <= 0 || a->Z <= 0 || a->H <= 0 || a->ldx < a->K1) return AIR_EINVAL;
    if (a->K1 != 256 || a->Z > 64) return AIR_ELIMIT;
    if ((a->Z & 1) || (a->H & 3) || (a->ldx & 3) || !aligned16(a->X) || !aligned16(a->Wml) || !aligned16(a->Wg)) return AIR_EALIGN;
    if (a->ldz != 0 && a->ldz < a->Z) return AIR_EINVAL;
    constexpr int K1 = 256;
    air_bottleneck_fwd_t k = *a;
    k.ldz = a->ldz > 0 ? a->ldz : a->Z;
    const dim3 grid((a->M + 15) / 16, (a->H + 63) / 64);
    if (a->exact_fp32) {
        if (2 * a->Z > 104) return AIR_ELIMIT;                      // Wml as it lies: rows of at most 104 + 4 floats of LDS
        return launch(bottleneck_fwd_f32_kernel<K1>, grid,
                      sizeof(float) * (16 * (K1 + FPAD) + K1 * (104 + FPAD) + (16 + 64) * (64 + FPAD)), stream, k);
    }
    const size_t lds = sizeof(unsigned short) * ((16 + 128) * (K1 + PAD) + (16 + 64) * (64 + PAD));
    // twin operands: all three or none; whole 16-byte pieces of X rows, 8-byte pieces of the weight rows
    const bool tw = a->X16 && a->Wml16 && a->Wg16 && aligned16(a->X16) && (a->ldx & 7) == 0 && aligned8(a->Wml16) && aligned8(a->Wg16);
    return tw ? launch(bottleneck_fwd_kernel<K1, true>, grid, lds, stream, k) : launch(bottleneck_fwd_kernel<K1, false>, grid, lds, stream, k);
}

extern "C" int air_vae_bottleneck_bwd(const air_bottleneck_bwd_t* a, void* stream) {
    if (!a || !a->dG || !a->Wg || !a->ml || !a->eps || !a->att || !a->dyn || !a->Wml || !a->x || !a->d_ml || !a->d_x) return AIR_EINVAL;
    if (a->M <= 0 || a->K1 <= 0 || a->Z <= 0 || a->H <= 0) return AIR_EINVAL;
    if (a->H != 256 || a->Z > 64) return AIR_ELIMIT;
    if ((a->Z & 1) || !aligned16(a->dG) || !aligned16(a->Wg) || !aligned16(a->Wml)) return AIR_EALIGN;
    constexpr int H = 256;
    const dim3 grid((a->M + 15) / 16, (a->K1 + 63) / 64);
    if (a->exact_fp32)
        return launch(bottleneck_bwd_f32_kernel<H>, grid, sizeof(float) * ((16 + 64) * (H + FPAD) + (16 + 64) * (128 + FPAD)), stream, *a);
    const size_t lds = sizeof(unsigned short) * ((16 + 64) * (H + PAD) + (16 + 64) * (128 + PAD));
    const bool tw = a->dG16 && a->Wg16 && a->Wml16 && aligned16(a->dG16) && aligned16(a->Wg16) && aligned8(a->Wml16);
    return tw ? launch(bottleneck_bwd_kernel<H, true>, grid, lds, stream, *a) : launch(bottleneck_bwd_kernel<H, false>, grid, lds, stream, *a);
}
