// The CNN front-end of the reference (air/air_model.py:510-533) as launches of their own: three 5x5 SAME convolutions +
// ReLU with a 2x2 / stride-2 VALID max-pool after the first two, fp32, one input channel, F <= 8 filters, any canvas S >= 4
// (include/air_hip.h, "stand-alone CNN front-end").  air/cnn.py calls air_cnn_fwd / air_cnn_bwd; the train step of
// AIRModel(cnn=True) calls air_cnn_fwd and air_cnn_bwd_sq (the same backward, its batch reduction also leaving the
// sums of squares the global-norm clip needs).
//
// PLAN.  One workgroup per image, everything between the image and `out` stays in LDS.
//   forward (cnn_fwd_kernel, 256 threads): the zero-haloed image, the three kernels + biases and the zero-haloed pool1 /
//     pool2 planes live in LDS.  A thread owns one 2x2 pool window for ALL F filters (4 F accumulators): it loads the
//     6x6 input patch of a channel once (18 8-byte LDS reads: the planes are channel-planar with an even pitch, so lanes
//     of adjacent windows read adjacent 8-byte words -- conflict-free), reads every weight vector as 16-byte words at an
//     address all lanes share (LDS broadcast), applies ReLU, takes the FIRST maximum in row-major window order (code
//     2 dy + dx) and writes the pooled value into the next haloed plane: the un-pooled conv outputs never exist in memory.
//     conv3 has no pool: a thread owns one pixel for all F filters.
//   backward (cnn_bwd_kernel, 512 threads) per image, the partials of the image go to the caller's workspace:
//     A  g3 = d_out (out > 0) and pool2, haloed, in LDS;  dk3 / db3;  d_pool2 = conv of g3 with the flipped, transposed
//        k3, masked by pool2 > 0 and scattered to its argmax site of the (zeroed) un-pooled plane G2 (windows are disjoint)
//     B  dk2 / db2 from G2 and the haloed pool1;  d_pool1 = conv of G2 with the flipped, transposed k2, masked by
//        pool1 > 0, kept COMPACT (one value + one code per window and channel: the un-pooled S x S x F plane would not fit)
//     C  dk1 / db1 as sums over the windows at their argmax sites;  d_images (only when asked for) gathers, per pixel,
//        from the <= 3x3 windows whose site can reach it.
//   cnn_reduce_kernel: one thread per variable element sums the per-image partials in ascending image order.
//   cnn_reduce_sq_kernel (air_cnn_bwd_sq): the same sums, same order, same bits; every workgroup also leaves the sum of
//     squares of the <= 256 elements it stored (wave sums, then the four waves left to right: air_block_sum_256).
//
// ACCUMULATION ORDER (fixed; no executed reference graph exists for this block, so none is mirrored).  Every inner
// product is ONE chain of fmaf:
//   conv:    acc = bias; for ci ascending, ky ascending, kx ascending: acc = fmaf(in[ci][y+ky-2][x+kx-2], k[ky][kx][ci][f], acc)
//   d_pool*: acc = 0;    for f ascending, then the flipped taps (ky = 4..0, kx = 4..0): acc = fmaf(g[f][..], k[ky][kx][ci][f], acc)
//   dk2/dk3: acc = 0;    for y ascending, x ascending over the un-pooled plane: acc = fmaf(in[ci][y+ky-2][x+kx-2], g[f][y][x], acc)
//   dk1:     acc = 0;    for window y ascending, x ascending: acc = fmaf(image at the window's argmax site + tap, g, acc)
//   db*:     plain sums in the same (y, x) order;  d_images: windows (y, x) ascending, f ascending, fmaf
//   batch:   partial of image 0, then + image 1, + image 2, ...
// No atomics anywhere: two runs give the same bits.
//
// LIMITS.  1 <= F <= 8 (4 F accumulators per thread), S >= 4, and both kernels' LDS (cnn_lds, the one function the
// launches size themselves with) must fit AIR_LDS_LIMIT: S <= 77 at F = 8 .. S <= 128 at F <= 2.  Either entry point
// refuses (AIR_ELIMIT) what the other could not run, so a forward that ran can be differentiated.
#include "air_common.h"

AIR_STAMPS_READER(air_debug_stamps_cnn)     // debug builds only (-DAIR_STAMPS): forward stamps 0..4, backward 10..17

namespace {

constexpr int FWD_NT = 256, BWD_NT = 512, MAX_F = 8, MAX_S = 128;

// An offset of 0 the optimiser cannot see through.  The weight reads of a conv are invariant across the windows a
// thread loops over; hoisted out of that loop they would occupy 25 F registers (conv1) for the whole kernel.
__device__ __forceinline__ int opaque_zero() { int o = 0; asm volatile("" : "+v"(o)); return o; }

__host__ __device__ inline int r2(int v) { return (v + 1) & ~1; }
__host__ __device__ inline int r4(int v) { return (v + 3) & ~3; }

// Offsets, in floats, of the LDS regions of both kernels.  Haloed planes: (n + 4) rows of an even pitch, channel-planar.
struct CnnLds {
    int S1, S2, FP, IP, P1, P2, img_n, pl1, pl2;      // pooled sizes, padded F, pitches, plane sizes
    int f_w1, f_w2, f_w3, f_bias, f_img, f_p1, f_p2, f_total;
    int b_w3, b_w2, b_k1, b_r1, b_r2, b_r4, b_code, b_total;    // r1: g3h | p2h, then the image;  r2: G2;  r4: p1h, then d1 | codes
};
__host__ __device__ inline CnnLds cnn_lds(int S, int F) {
    CnnLds L;
    L.S1 = S >> 1; L.S2 = L.S1 >> 1; L.FP = r4(F);
    L.IP = r2(S + 4); L.P1 = r2(L.S1 + 4); L.P2 = r2(L.S2 + 4);
    L.img_n = r4(L.IP * (S + 4)); L.pl1 = L.P1 * (L.S1 + 4); L.pl2 = L.P2 * (L.S2 + 4);
    const int wn = r4(25 * F * L.FP);
    L.f_w1 = 0; L.f_w2 = r4(25 * L.FP); L.f_w3 = L.f_w2 + wn; L.f_bias = L.f_w3 + wn;
    L.f_img = L.f_bias + r4(3 * L.FP); L.f_p1 = L.f_img + L.img_n; L.f_p2 = L.f_p1 + r4(F * L.pl1);
    L.f_total = L.f_p2 + r4(F * L.pl2);
    L.b_w3 = 0; L.b_w2 = wn; L.b_k1 = 2 * wn; L.b_r1 = L.b_k1 + r4(25 * L.FP);
    const int r1 = 2 * r4(F * L.pl2) > L.img_n ? 2 * r4(F * L.pl2) : L.img_n;
    L.b_r2 = L.b_r1 + r1; L.b_r4 = L.b_r2 + r4(F * L.pl1);
    const int d1 = r4(F * L.S1 * L.S1);                         // compact d_pre1, then one code byte per value
    const int r4n = d1 + r4((F * L.S1 * L.S1 + 3) / 4) > r4(F * L.pl1) ? d1 + r4((F * L.S1 * L.S1 + 3) / 4) : r4(F * L.pl1);
    L.b_code = L.b_r4 + d1; L.b_total = L.b_r4 + r4n;
    return L;
}

// per-image partials in the workspace: dk1 | db1 | dk2 | db2 | dk3 | db3
__host__ __device__ inline int cnn_num_partials(int F) { return 25 * F + 50 * F * F + 3 * F; }

// kernel [25][cin][F] of global memory -> [25][cin][FP] of LDS (zero padding), or with `flip` the operand of the data
// gradient: [tap'][f][ciP] = k[24 - tap'][ci][f] (cin == F there)
template <int F, int NT>
__device__ __forceinline__ void stage_kernel(float* dst, const float* __restrict__ k, int cin, bool flip) {
    constexpr int FP = (F + 3) & ~3;
    for (int i = threadIdx.x; i < 25 * cin * FP; i += NT) {
        const int c = i % FP, r = i / FP;
        float v = 0.0f;
        if (c < F) {
            if (!flip) v = k[r * F + c];
            else { const int f = r % F, t = r / F; v = k[((24 - t) * F + c) * F + f]; }
        }
        dst[i] = v;
    }
}

// 2x2 window of outputs x CO output channels: `in` points at the top-left of the window's 6x6 patch in plane 0
template <int CO>
__device__ __forceinline__ void conv_win(const float* in, int pitch, int plane, int cin, const float* w, float (&acc)[4][CO]) {
    constexpr int COP = (CO + 3) & ~3;
    w += opaque_zero();
#pragma unroll 1                                     // (cin is a constant after inlining: unrolled, every channel's patch and weights were live at once)
    for (int ci = 0; ci < cin; ++ci) {
        float p[6][6];
        const float* q = in + ci * plane;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float2 v = *reinterpret_cast<const float2*>(q + r * pitch + 2 * c);
                p[r][2 * c] = v.x; p[r][2 * c + 1] = v.y;
            }
        }
#pragma unroll
        for (int ky = 0; ky < 5; ++ky) {
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                float wv[COP];
                const float4* w4 = reinterpret_cast<const float4*>(w + ((ky * 5 + kx) * cin + ci) * COP);
#pragma unroll
                for (int j = 0; j < COP / 4; ++j) { const float4 t = w4[j]; wv[4 * j] = t.x; wv[4 * j + 1] = t.y; wv[4 * j + 2] = t.z; wv[4 * j + 3] = t.w; }
#pragma unroll
                for (int f = 0; f < CO; ++f) {
                    acc[0][f] = __builtin_fmaf(p[ky][kx], wv[f], acc[0][f]);
                    acc[1][f] = __builtin_fmaf(p[ky][kx + 1], wv[f], acc[1][f]);
                    acc[2][f] = __builtin_fmaf(p[ky + 1][kx], wv[f], acc[2][f]);
                    acc[3][f] = __builtin_fmaf(p[ky + 1][kx + 1], wv[f], acc[3][f]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);       // one row of taps' weights in flight, not all 25: 5 COP registers
        }
    }
}

// one pixel x CO output channels: `in` points at the top-left of the pixel's 5x5 patch in plane 0
template <int CO>
__device__ __forceinline__ void conv_pix(const float* in, int pitch, int plane, int cin, const float* w, float (&acc)[CO]) {
    constexpr int COP = (CO + 3) & ~3;
    w += opaque_zero();
#pragma unroll 1                                     // (cin is a constant after inlining: unrolled, every channel's patch and weights were live at once)
    for (int ci = 0; ci < cin; ++ci) {
        float p[5][5];
        const float* q = in + ci * plane;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
#pragma unroll
            for (int c = 0; c < 5; ++c) p[r][c] = q[r * pitch + c];
        }
#pragma unroll
        for (int t = 0; t < 25; ++t) {
            float wv[COP];
            const float4* w4 = reinterpret_cast<const float4*>(w + (t * cin + ci) * COP);
#pragma unroll
            for (int j = 0; j < COP / 4; ++j) { const float4 v = w4[j]; wv[4 * j] = v.x; wv[4 * j + 1] = v.y; wv[4 * j + 2] = v.z; wv[4 * j + 3] = v.w; }
#pragma unroll
            for (int f = 0; f < CO; ++f) acc[f] = __builtin_fmaf(p[t / 5][t % 5], wv[f], acc[f]);
            if (t % 5 == 4) __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// ReLU, then the first maximum of the window in row-major order; the pooled value goes to the haloed LDS plane of every
// channel and, with the saved tensors, to global memory with its code
template <int F>
__device__ __forceinline__ void pool_store(const float (&acc)[4][F], float* plane0, int plane, float* gp, uint8_t* ga) {
#pragma unroll
    for (int f = 0; f < F; ++f) {
        float best = fmaxf(acc[0][f], 0.0f);
        int code = 0;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            const float v = fmaxf(acc[j][f], 0.0f);
            if (v > best) { best = v; code = j; }
        }
        plane0[f * plane] = best;
        if (gp) { gp[f] = best; ga[f] = (uint8_t)code; }
    }
}

template <int F>
__global__ __launch_bounds__(FWD_NT) void cnn_fwd_kernel(const air_cnn_fwd_t a) {
    constexpr int FP = (F + 3) & ~3, NT = FWD_NT;
    extern __shared__ __align__(16) float lds[];
    const int S = a.S, tid = threadIdx.x;
    const CnnLds L = cnn_lds(S, F);
    const int S1 = L.S1, S2 = L.S2;
    const size_t b = blockIdx.x;
    AIR_STAMP(0);
    stage_kernel<F, NT>(lds + L.f_w1, a.k1, 1, false);
    stage_kernel<F, NT>(lds + L.f_w2, a.k2, F, false);
    stage_kernel<F, NT>(lds + L.f_w3, a.k3, F, false);
    if (tid < 3 * FP) {
        const int l = tid / FP, f = tid % FP;
        const float* bias = l == 0 ? a.b1 : l == 1 ? a.b2 : a.b3;
        lds[L.f_bias + tid] = f < F ? bias[f] : 0.0f;
    }
    const float* im = a.images + b * S * S;
    for (int i = tid; i < L.IP * (S + 4); i += NT) {
        const int y = i / L.IP - 2, x = i % L.IP - 2;
        lds[L.f_img + i] = ((unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S) ? im[y * S + x] : 0.0f;
    }
    for (int i = L.f_p1 + tid; i < L.f_total; i += NT) lds[i] = 0.0f;
    __syncthreads();
    AIR_STAMP(1);
    const bool save = a.pool1 != nullptr;
    // conv1 + ReLU + pool1
    for (int it = tid; it < S1 * S1; it += NT) {
        const int wy = it / S1, wx = it - wy * S1;
        float acc[4][F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[0][f] = acc[1][f] = acc[2][f] = acc[3][f] = lds[L.f_bias + f];
        conv_win<F>(lds + L.f_img + 2 * wy * L.IP + 2 * wx, L.IP, 0, 1, lds + L.f_w1, acc);
        const size_t g = (b * S1 * S1 + it) * F;
        pool_store<F>(acc, lds + L.f_p1 + (wy + 2) * L.P1 + wx + 2, L.pl1, save ? a.pool1 + g : nullptr, save ? a.arg1 + g : nullptr);
    }
    __syncthreads();
    AIR_STAMP(2);
    // conv2 + ReLU + pool2
    for (int it = tid; it < S2 * S2; it += NT) {
        const int wy = it / S2, wx = it - wy * S2;
        float acc[4][F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[0][f] = acc[1][f] = acc[2][f] = acc[3][f] = lds[L.f_bias + FP + f];
        conv_win<F>(lds + L.f_p1 + 2 * wy * L.P1 + 2 * wx, L.P1, L.pl1, F, lds + L.f_w2, acc);
        const size_t g = (b * S2 * S2 + it) * F;
        pool_store<F>(acc, lds + L.f_p2 + (wy + 2) * L.P2 + wx + 2, L.pl2, save ? a.pool2 + g : nullptr, save ? a.arg2 + g : nullptr);
    }
    __syncthreads();
    AIR_STAMP(3);
    // conv3 + ReLU
    for (int it = tid; it < S2 * S2; it += NT) {
        const int y = it / S2, x = it - y * S2;
        float acc[F];
#pragma unroll
        for (int f = 0; f < F; ++f) acc[f] = lds[L.f_bias + 2 * FP + f];
        conv_pix<F>(lds + L.f_p2 + y * L.P2 + x, L.P2, L.pl2, F, lds + L.f_w3, acc);
        float* o = a.out + (b * S2 * S2 + it) * F;
#pragma unroll
        for (int f = 0; f < F; ++f) o[f] = fmaxf(acc[f], 0.0f);
    }
    AIR_STAMP(4);
}

// dk[ky][0..4][ci][f] of one (ci, f, ky): P at plane ci, row ky of the haloed input; G at the interior of plane f of the
// haloed gradient; both n x n with the same pitch.  A sliding window over x: two LDS reads per five fmaf.
__device__ __forceinline__ void wgrad_row5(const float* P, const float* G, int n, int pitch, float (&acc)[5]) {
    for (int y = 0; y < n; ++y) {
        const float* pr = P + y * pitch;
        const float* gr = G + y * pitch;
        float p0 = pr[0], p1 = pr[1], p2 = pr[2], p3 = pr[3];
#pragma unroll 4
        for (int x = 0; x < n; ++x) {
            const float p4 = pr[x + 4], g = gr[x];
            acc[0] = __builtin_fmaf(p0, g, acc[0]);
            acc[1] = __builtin_fmaf(p1, g, acc[1]);
            acc[2] = __builtin_fmaf(p2, g, acc[2]);
            acc[3] = __builtin_fmaf(p3, g, acc[3]);
            acc[4] = __builtin_fmaf(p4, g, acc[4]);
            p0 = p1; p1 = p2; p2 = p3; p3 = p4;
        }
    }
}

// dk [25][F][F] and db [F] of a layer with F input channels into the image's partials: items (ci, f, ky), then f
template <int F, int NT>
__device__ __forceinline__ void wgrad_layer(const float* Ph, const float* Gh, int n, int pitch, int plane, float* dk, float* db) {
    for (int it = threadIdx.x; it < 5 * F * F + F; it += NT) {
        if (it < 5 * F * F) {
            const int ky = it / (F * F), r = it - ky * F * F, ci = r / F, f = r - ci * F;
            float acc[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            wgrad_row5(Ph + ci * plane + ky * pitch, Gh + f * plane + 2 * pitch + 2, n, pitch, acc);
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) dk[((ky * 5 + kx) * F + ci) * F + f] = acc[kx];
        } else {
            const int f = it - 5 * F * F;
            const float* G = Gh + f * plane + 2 * pitch + 2;
            float s = 0.0f;
            for (int y = 0; y < n; ++y) {
#pragma unroll 4
                for (int x = 0; x < n; ++x) s += G[y * pitch + x];
            }
            db[f] = s;
        }
    }
}

template <int F>
__global__ __launch_bounds__(BWD_NT) void cnn_bwd_kernel(const air_cnn_bwd_t a) {
    constexpr int FP = (F + 3) & ~3, NT = BWD_NT;
    extern __shared__ __align__(16) float lds[];
    const int S = a.S, tid = threadIdx.x;
    const CnnLds L = cnn_lds(S, F);
    const int S1 = L.S1, S2 = L.S2;
    const size_t b = blockIdx.x;
    float* ws = a.workspace + b * cnn_num_partials(F);
    float* dk1 = ws; float* db1 = dk1 + 25 * F; float* dk2 = db1 + F; float* db2 = dk2 + 25 * F * F;
    float* dk3 = db2 + F; float* db3 = dk3 + 25 * F * F;
    float* g3h = lds + L.b_r1; float* p2h = g3h + r4(F * L.pl2); float* G2 = lds + L.b_r2; float* p1h = lds + L.b_r4;
    float* imgh = lds + L.b_r1; float* d1c = lds + L.b_r4;
    uint8_t* code1 = reinterpret_cast<uint8_t*>(lds + L.b_code);

    // ---- stage: flipped kernels, g3 = d_out (out > 0), pool2 and pool1 with their halos, a zeroed G2
    AIR_STAMP(10);
    stage_kernel<F, NT>(lds + L.b_w3, a.k3, F, true);
    stage_kernel<F, NT>(lds + L.b_w2, a.k2, F, true);
    stage_kernel<F, NT>(lds + L.b_k1, a.k1, 1, false);
    {
        const float* go = a.d_out + b * S2 * S2 * F;
        const float* oo = a.out + b * S2 * S2 * F;
        const float* pp = a.pool2 + b * S2 * S2 * F;
        for (int i = tid; i < F * L.pl2; i += NT) {
            const int f = i / L.pl2, r = i - f * L.pl2, y = r / L.P2 - 2, x = r % L.P2 - 2;
            float g = 0.0f, p = 0.0f;
            if ((unsigned)y < (unsigned)S2 && (unsigned)x < (unsigned)S2) {
                const int j = (y * S2 + x) * F + f;
                g = oo[j] > 0.0f ? go[j] : 0.0f;
                p = pp[j];
            }
            g3h[i] = g; p2h[i] = p;
        }
        const float* p1 = a.pool1 + b * S1 * S1 * F;
        for (int i = tid; i < F * L.pl1; i += NT) {
            const int f = i / L.pl1, r = i - f * L.pl1, y = r / L.P1 - 2, x = r % L.P1 - 2;
            p1h[i] = ((unsigned)y < (unsigned)S1 && (unsigned)x < (unsigned)S1) ? p1[(y * S1 + x) * F + f] : 0.0f;
            G2[i] = 0.0f;
        }
    }
    __syncthreads();
    AIR_STAMP(11);

    // ---- A: dk3 / db3, and d_pool2 scattered to the argmax sites of G2
    wgrad_layer<F, NT>(p2h, g3h, S2, L.P2, L.pl2, dk3, db3);
    AIR_STAMP(12);
    for (int it = tid; it < S2 * S2; it += NT) {
        const int y = it / S2, x = it - y * S2;
        float acc[F];
#pragma unroll
        for (int c = 0; c < F; ++c) acc[c] = 0.0f;
        conv_pix<F>(g3h + y * L.P2 + x, L.P2, L.pl2, F, lds + L.b_w3, acc);
        const uint8_t* code = a.arg2 + (b * S2 * S2 + it) * F;
#pragma unroll
        for (int c = 0; c < F; ++c) {
            const int k = code[c] & 3;
            const float g = p2h[c * L.pl2 + (y + 2) * L.P2 + x + 2] > 0.0f ? acc[c] : 0.0f;
            G2[c * L.pl1 + (2 * y + (k >> 1) + 2) * L.P1 + 2 * x + (k & 1) + 2] = g;
        }
    }
    __syncthreads();
    AIR_STAMP(13);

    // ---- B: dk2 / db2;  the image replaces g3 / pool2
    wgrad_layer<F, NT>(p1h, G2, S1, L.P1, L.pl1, dk2, db2);
    {
        const float* im = a.images + b * S * S;
        for (int i = tid; i < L.IP * (S + 4); i += NT) {
            const int y = i / L.IP - 2, x = i % L.IP - 2;
            imgh[i] = ((unsigned)y < (unsigned)S && (unsigned)x < (unsigned)S) ? im[y * S + x] : 0.0f;
        }
    }
    __syncthreads();
    AIR_STAMP(14);
    // d_pool1, masked, compact (it replaces the haloed pool1)
    for (int it = tid; it < S1 * S1; it += NT) {
        const int y = it / S1, x = it - y * S1;
        float acc[F];
#pragma unroll
        for (int c = 0; c < F; ++c) acc[c] = 0.0f;
        conv_pix<F>(G2 + y * L.P1 + x, L.P1, L.pl1, F, lds + L.b_w2, acc);
        const float* pv = a.pool1 + (b * S1 * S1 + it) * F;
        const uint8_t* code = a.arg1 + (b * S1 * S1 + it) * F;
#pragma unroll
        for (int c = 0; c < F; ++c) {
            d1c[c * S1 * S1 + it] = pv[c] > 0.0f ? acc[c] : 0.0f;
            code1[c * S1 * S1 + it] = code[c] & 3;
        }
    }
    __syncthreads();
    AIR_STAMP(15);

    // ---- C: dk1 / db1 over the windows at their argmax sites; d_images when asked for
    for (int it = tid; it < 25 * F + F; it += NT) {
        if (it < 25 * F) {
            const int t = it / F, f = it - t * F, ky = t / 5, kx = t - ky * 5;
            const float* d = d1c + f * S1 * S1;
            const uint8_t* cd = code1 + f * S1 * S1;
            const float* q = imgh + ky * L.IP + kx;
            float acc = 0.0f;
            for (int y = 0; y < S1; ++y) {
#pragma unroll 4                                                    // the code read and the image read it addresses, four in flight
                for (int x = 0; x < S1; ++x) {
                    const int k = cd[y * S1 + x];
                    acc = __builtin_fmaf(q[(2 * y + (k >> 1)) * L.IP + 2 * x + (k & 1)], d[y * S1 + x], acc);
                }
            }
            dk1[it] = acc;
        } else {
            const int f = it - 25 * F;
            float s = 0.0f;
#pragma unroll 4
            for (int i = 0; i < S1 * S1; ++i) s += d1c[f * S1 * S1 + i];
            db1[f] = s;
        }
    }
    AIR_STAMP(16);
    if (a.d_images) {
        const float* k1 = lds + L.b_k1;
        float* di = a.d_images + b * S * S;
        for (int it = tid; it < S * S; it += NT) {
            const int Y = it / S, X = it - Y * S;
            const int wy0 = (Y > 2 ? Y - 2 : 0) >> 1, wy1 = min((Y + 2) >> 1, S1 - 1);
            const int wx0 = (X > 2 ? X - 2 : 0) >> 1, wx1 = min((X + 2) >> 1, S1 - 1);
            float acc = 0.0f;
            for (int wy = wy0; wy <= wy1; ++wy)
                for (int wx = wx0; wx <= wx1; ++wx) {
#pragma unroll
                    for (int f = 0; f < F; ++f) {
                        const int k = code1[f * S1 * S1 + wy * S1 + wx];
                        const int ky = Y - (2 * wy + (k >> 1)) + 2, kx = X - (2 * wx + (k & 1)) + 2;
                        if ((unsigned)ky < 5u && (unsigned)kx < 5u)
                            acc = __builtin_fmaf(d1c[f * S1 * S1 + wy * S1 + wx], k1[(ky * 5 + kx) * FP + f], acc);
                    }
                }
            di[it] = acc;
        }
    }
    AIR_STAMP(17);
}

// sum of the per-image partials in ascending image order, one thread per variable element
__global__ __launch_bounds__(256) void cnn_reduce_kernel(const float* __restrict__ ws, int B, int F, float* d_k1, float* d_b1,
                                                         float* d_k2, float* d_b2, float* d_k3, float* d_b3) {
    const int np = cnn_num_partials(F);
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= np) return;
    float s = ws[j];
    for (int b = 1; b < B; ++b) s += ws[(size_t)b * np + j];
    const int n1 = 25 * F, n2 = 25 * F * F;
    int r = j;
    if (r < n1) { d_k1[r] = s; return; }
    r -= n1;
    if (r < F) { d_b1[r] = s; return; }
    r -= F;
    if (r < n2) { d_k2[r] = s; return; }
    r -= n2;
    if (r < F) { d_b2[r] = s; return; }
    r -= F;
    if (r < n2) { d_k3[r] = s; return; }
    d_b3[r - n2] = s;
}

// where element j of an image's partials (dk1 | db1 | dk2 | db2 | dk3 | db3) lives among the six gradients
__device__ __forceinline__ float* cnn_grad_slot(int j, int F, float* d_k1, float* d_b1, float* d_k2, float* d_b2, float* d_k3, float* d_b3) {
    const int n1 = 25 * F, n2 = 25 * F * F;
    if (j < n1) return d_k1 + j;
    j -= n1;
    if (j < F) return d_b1 + j;
    j -= F;
    if (j < n2) return d_k2 + j;
    j -= n2;
    if (j < F) return d_b2 + j;
    j -= F;
    if (j < n2) return d_k3 + j;
    return d_b3 + (j - n2);
}

// cnn_reduce_kernel's sums (image 0, then + image 1, ...: the same bits) and, per workgroup, the sum of squares of the
// elements it stored: a thread past the last element contributes an exact zero.  Workgroup i writes sq_partials[i].
__global__ __launch_bounds__(256) void cnn_reduce_sq_kernel(const float* __restrict__ ws, int B, int F, float* d_k1, float* d_b1,
                                                            float* d_k2, float* d_b2, float* d_k3, float* d_b3,
                                                            float* __restrict__ sq_partials) {
    __shared__ float red[4];
    const int np = cnn_num_partials(F);
    const int j = blockIdx.x * 256 + threadIdx.x;
    float sq = 0.0f;
    if (j < np) {
        float s = ws[j];
#pragma unroll 8                                     // eight images' loads in flight; the adds keep their order (same bits)
        for (int b = 1; b < B; ++b) s += ws[(size_t)b * np + j];
        *cnn_grad_slot(j, F, d_k1, d_b1, d_k2, d_b2, d_k3, d_b3) = s;
        sq = s * s;
    }
    sq = air_block_sum_256(sq, red);
    if (threadIdx.x == 0) sq_partials[blockIdx.x] = sq;
}

constexpr int cnn_reduce_blocks(int F) { return (25 * F + 50 * F * F + 3 * F + 255) / 256; }

// AIR_EINVAL / AIR_ELIMIT of a (B, S, F), the same answer for both entry points and the workspace query
int cnn_check(int B, int S, int F) {
    if (B < 1 || S < 4 || F < 1) return AIR_EINVAL;
    if (F > MAX_F || S > MAX_S) return AIR_ELIMIT;
    const CnnLds L = cnn_lds(S, F);
    const size_t need = sizeof(float) * (size_t)(L.f_total > L.b_total ? L.f_total : L.b_total);
    return need > AIR_LDS_LIMIT ? AIR_ELIMIT : 0;
}

template <int F>
int launch_fwd(const air_cnn_fwd_t* a, void* stream) {
    const size_t bytes = sizeof(float) * (size_t)cnn_lds(a->S, F).f_total;
    if (int rc = air_grant_lds(reinterpret_cast<const void*>(&cnn_fwd_kernel<F>), bytes)) return rc;
    hipLaunchKernelGGL(cnn_fwd_kernel<F>, dim3(a->B), dim3(FWD_NT), bytes, air_stream(stream), *a);
    AIR_CHECK_LAUNCH();
    return 0;
}

// sq_partials == NULL: air_cnn_bwd (cnn_reduce_kernel); else air_cnn_bwd_sq (cnn_reduce_sq_kernel)
template <int F>
int launch_bwd(const air_cnn_bwd_t* a, float* sq_partials, void* stream) {
    const size_t bytes = sizeof(float) * (size_t)cnn_lds(a->S, F).b_total;
    if (int rc = air_grant_lds(reinterpret_cast<const void*>(&cnn_bwd_kernel<F>), bytes)) return rc;
    hipLaunchKernelGGL(cnn_bwd_kernel<F>, dim3(a->B), dim3(BWD_NT), bytes, air_stream(stream), *a);
    AIR_CHECK_LAUNCH();
    if (sq_partials)
        hipLaunchKernelGGL(cnn_reduce_sq_kernel, dim3(cnn_reduce_blocks(F)), dim3(256), 0, air_stream(stream),
                           a->workspace, a->B, F, a->d_k1, a->d_b1, a->d_k2, a->d_b2, a->d_k3, a->d_b3, sq_partials);
    else
        hipLaunchKernelGGL(cnn_reduce_kernel, dim3((cnn_num_partials(F) + 255) / 256), dim3(256), 0, air_stream(stream),
                           a->workspace, a->B, F, a->d_k1, a->d_b1, a->d_k2, a->d_b2, a->d_k3, a->d_b3);
    AIR_CHECK_LAUNCH();
    return 0;
}

int cnn_bwd_dispatch(const air_cnn_bwd_t* a, float* sq_partials, void* stream) {
    if (!a || !a->d_out || !a->out || !a->images || !a->pool1 || !a->pool2 || !a->arg1 || !a->arg2 || !a->k1 || !a->k2 ||
        !a->k3 || !a->workspace || !a->d_k1 || !a->d_b1 || !a->d_k2 || !a->d_b2 || !a->d_k3 || !a->d_b3) return AIR_EINVAL;
    if (int rc = cnn_check(a->B, a->S, a->F)) return rc;
    switch (a->F) {
        case 1: return launch_bwd<1>(a, sq_partials, stream);
        case 2: return launch_bwd<2>(a, sq_partials, stream);
        case 3: return launch_bwd<3>(a, sq_partials, stream);
        case 4: return launch_bwd<4>(a, sq_partials, stream);
        case 5: return launch_bwd<5>(a, sq_partials, stream);
        case 6: return launch_bwd<6>(a, sq_partials, stream);
        case 7: return launch_bwd<7>(a, sq_partials, stream);
        default: return launch_bwd<8>(a, sq_partials, stream);
    }
}

}  // namespace

extern "C" int64_t air_cnn_workspace_floats(int B, int S, int F) {
    if (int rc = cnn_check(B, S, F)) return rc;
    return (int64_t)B * cnn_num_partials(F);
}

extern "C" int air_cnn_fwd(const air_cnn_fwd_t* a, void* stream) {
    if (!a || !a->images || !a->k1 || !a->b1 || !a->k2 || !a->b2 || !a->k3 || !a->b3 || !a->out) return AIR_EINVAL;
    const int saved = (a->pool1 != nullptr) + (a->pool2 != nullptr) + (a->arg1 != nullptr) + (a->arg2 != nullptr);
    if (saved != 0 && saved != 4) return AIR_EINVAL;               // the four saved tensors come together or not at all
    if (int rc = cnn_check(a->B, a->S, a->F)) return rc;
    switch (a->F) {
        case 1: return launch_fwd<1>(a, stream);
        case 2: return launch_fwd<2>(a, stream);
        case 3: return launch_fwd<3>(a, stream);
        case 4: return launch_fwd<4>(a, stream);
        case 5: return launch_fwd<5>(a, stream);
        case 6: return launch_fwd<6>(a, stream);
        case 7: return launch_fwd<7>(a, stream);
        default: return launch_fwd<8>(a, stream);
    }
}

extern "C" int air_cnn_bwd(const air_cnn_bwd_t* a, void* stream) { return cnn_bwd_dispatch(a, nullptr, stream); }

extern "C" int air_cnn_num_sq_partials(int F) {
    if (F < 1) return AIR_EINVAL;
    if (F > MAX_F) return AIR_ELIMIT;
    return cnn_reduce_blocks(F);
}

extern "C" int air_cnn_bwd_sq(const air_cnn_bwd_t* a, float* sq_partials, void* stream) {
    if (!sq_partials) return AIR_EINVAL;
    return cnn_bwd_dispatch(a, sq_partials, stream);
}
