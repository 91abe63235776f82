// The write backward of the AIR loop (window <- d loss / d canvas; air_model.py:351-366 under tf.gradients,
// transformer.py:56-171): the exact adjoint, the op order of the reference's saved graph (the default: one sequential fp32
// accumulator per window pixel, on the LDS atomic pipe for the four corner slots) and the carried order; the backward of the
// generic transformer, for one channel and for [B,H,W,C] inputs with several transforms per image; the probe of the LDS
// atomic pipe's lane order that the graph order rests on.  Shared geometry: air_sampler_common.h.
#include "air_sampler_common.h"

AIR_STAMPS_READER(air_debug_stamps_wb)
// per-workgroup phase stamps of the graph-order write backward (debug builds only): [workgroup][8]
#ifdef AIR_STAMPS
static __device__ unsigned long long air_stamps_wg[4096 * 8];
extern "C" int air_debug_stamps_wg(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(air_stamps_wg), sizeof(unsigned long long) * (n < 4096 * 8 ? n : 4096 * 8));
}
#define AIR_STAMP_WG(i) do { if (threadIdx.x == 0) air_stamps_wg[((blockIdx.y * gridDim.x + blockIdx.x) & 4095) * 8 + (i)] = wall_clock64(); } while (0)
#define AIR_STAMP_WG_T(i, t) do { if (threadIdx.x == (t)) air_stamps_wg[((blockIdx.y * gridDim.x + blockIdx.x) & 4095) * 8 + (i)] = wall_clock64(); } while (0)
// accumulating form (large canvases: four passes per workgroup): slot i += now - t0, and plain values
#define AIR_STAMP_WG_ADD(i, t0) do { if (threadIdx.x == 0) air_stamps_wg[((blockIdx.y * gridDim.x + blockIdx.x) & 4095) * 8 + (i)] += wall_clock64() - (t0); } while (0)
#define AIR_STAMP_WG_SET(i, v) do { if (threadIdx.x == 0) air_stamps_wg[((blockIdx.y * gridDim.x + blockIdx.x) & 4095) * 8 + (i)] = (unsigned long long)(v); } while (0)
#define AIR_NOW() wall_clock64()
#else
#define AIR_STAMP_WG(i) do { } while (0)
#define AIR_STAMP_WG_T(i, t) do { } while (0)
#define AIR_STAMP_WG_ADD(i, t0) do { } while (0)
#define AIR_STAMP_WG_SET(i, v) do { } while (0)
#define AIR_NOW() 0ull
#endif

namespace {

typedef __attribute__((address_space(3))) float air_lds_float;
// no-return LDS float add (inline asm: no compare-and-swap loop may be substituted)
__device__ __forceinline__ void lds_fadd(float* p, float v) {
    asm volatile("ds_add_f32 %0, %1" :: "v"((unsigned)(size_t)(air_lds_float*)p), "v"(v) : "memory");
}

// ---------------------------------------------------------------------------
// generic transformer backward (any theta): gradients wrt the input image U and wrt theta, in the
// op order of the reference's graph (transformer.py:56-171 differentiated by tf.gradients; node
// orders from model/air-model.meta):
//   * d theta: per output pixel, graph_dxy's AddN order for the coordinate gradients, then the
//     MatMul_grad contraction over the output pixels with (x_t, y_t, 1);
//   * d U: the four Gather gradients concatenated and reduced by one UnsortedSegmentSum -- every input
//     pixel is ONE fp32 accumulator receiving its a-terms in output-pixel order, then b, c, d.  For an
//     arbitrary theta the contributors of a slot are not a rectangle, so the accumulation is done
//     where the hardware already provides that order: one wave walks the 4*Ho*Wo terms in sequence,
//     64 per ds_add_f32; gfx950's LDS applies the lanes of an instruction in ascending order and a
//     wave's instructions in program order (tools/exp/lds_atomic_order.hip), i.e. exactly the scatter
//     order of the reference's CPU kernel.  One workgroup per image; U and d U live in LDS.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void transformer_bwd_kernel(
    const float* __restrict__ U, const float* __restrict__ theta, const float* __restrict__ d_out,
    float* __restrict__ d_U, float* __restrict__ d_theta, int Hi, int Wi, int Ho, int Wo, int lds_ordered)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NI = Hi * Wi, NO = Ho * Wo;
    float* sh_red = smem;                      // [32]
    float* sh_th = smem + 32;                  // [8]
    float* sh_U = smem + 40;                   // [NI]
    float* sh_dU = sh_U + ((NI + 3) & ~3);     // [NI]
    const float* img = U + (size_t)b * NI;
    const float* g = d_out + (size_t)b * NO;
    if (tid < 6) sh_th[tid] = theta[(size_t)b * 6 + tid];
    for (int p = tid; p < NI; p += THREADS) { sh_U[p] = img[p]; sh_dU[p] = 0.0f; }
    __syncthreads();
    if (d_theta) {
        float s6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int p = tid; p < NO; p += THREADS) {
            const GenTap t = generic_tap(sh_th, p / Wo, p % Wo, Hi, Wi, Ho, Wo);
            const float Ia = sh_U[t.y0 * Wi + t.x0], Ib = sh_U[t.y1 * Wi + t.x0];
            const float Ic = sh_U[t.y0 * Wi + t.x1], Id = sh_U[t.y1 * Wi + t.x1];
            generic_dtheta_pixel(t, g[p] * Ia, g[p] * Ib, g[p] * Ic, g[p] * Id, Hi, Wi, s6);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const float v = air_block_sum_256(s6[k], sh_red + 4 * k);
            if (tid == 0) d_theta[(size_t)b * 6 + k] = v;
        }
    }
    if (d_U) {
        __syncthreads();
        if (!lds_ordered) {
            // fallback for a part whose LDS atomics do not apply lanes in ascending order (lds_order_probe): ONE lane
            // walks the terms -- slow, but the reference's scatter order by construction
            if (tid == 0)
                for (int ph = 0; ph < 4; ++ph)
                    for (int p = 0; p < NO; ++p) {
                        const GenTap t = generic_tap(sh_th, p / Wo, p % Wo, Hi, Wi, Ho, Wo);
                        float wgt;
                        int idx;
                        generic_tap_term(t, ph, Wi, wgt, idx);
                        sh_dU[idx] = sh_dU[idx] + wgt * g[p];
                    }
        } else if (wave == 0) {
            for (int ph = 0; ph < 4; ++ph)
                for (int p0 = 0; p0 < NO; p0 += 64) {
                    const int p = p0 + lane;
                    if (p < NO) {
                        const GenTap t = generic_tap(sh_th, p / Wo, p % Wo, Hi, Wi, Ho, Wo);
                        float wgt;
                        int idx;
                        generic_tap_term(t, ph, Wi, wgt, idx);
                        lds_fadd(sh_dU + idx, wgt * g[p]);
                    }
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __syncthreads();
        float* dst = d_U + (size_t)b * NI;
        for (int p = tid; p < NI; p += THREADS) dst[p] = sh_dU[p];
    }
}

// ---------------------------------------------------------------------------
// generic transformer backward on [B,Hi,Wi,C] inputs with T transforms per image (air_transformer_nc_bwd): what
// tf.gradients builds for transformer.py:18-175 and, T > 1, for batch_transformer (:178-195).  One launch, two kinds
// of workgroup:
//   * d U, one workgroup per (image, group of up to NC_WAVES channels).  im_flat is [B*H*W, C] and the Gather gradients
//     carry rows of C values into the UnsortedSegmentSum, so a channel is the single-channel stream above on its own
//     plane: wave k of the workgroup walks the 4*Ho*Wo terms of channel c0 + k into that channel's plane of LDS -- the
//     waves that sit idle in transformer_bwd_kernel -- and a plane only ever sees the adds of one wave, in program
//     order.  The tf.gather of batch_transformer has one more UnsortedSegmentSum as its gradient, over the rows of an
//     image in ascending order: every transform's d U is completed from zero, then added to the image's, t = 0, 1, ...
//     (NOT one accumulator carried across the transforms);
//   * d theta, one workgroup per row.  The weights are shared by the channels: the graph reduces g * I over the channel
//     axis (ascending c, from the c = 0 product) before the AddN legs; from there on the arithmetic and the reduction
//     of transformer_bwd_kernel, so at C = 1 the same bits.  U comes from memory: C contiguous floats per tap.
// ---------------------------------------------------------------------------
constexpr int NC_WAVES = THREADS / 64;
__device__ __forceinline__ void transformer_nc_dtheta(
    const float* __restrict__ img, const float* __restrict__ theta_row, const float* __restrict__ g, float* __restrict__ d_theta_row,
    int Hi, int Wi, int C, int Ho, int Wo, float* sh_red)
{
    const int tid = threadIdx.x, NO = Ho * Wo;
    float th[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) th[k] = theta_row[k];
    float s6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = tid; p < NO; p += THREADS) {
        const GenTap t = generic_tap(th, p / Wo, p % Wo, Hi, Wi, Ho, Wo);
        const float* pa = img + (size_t)(t.y0 * Wi + t.x0) * C;
        const float* pb = img + (size_t)(t.y1 * Wi + t.x0) * C;
        const float* pc = img + (size_t)(t.y0 * Wi + t.x1) * C;
        const float* pd = img + (size_t)(t.y1 * Wi + t.x1) * C;
        const float* gp = g + (size_t)p * C;
        // Sum over the channel axis of mul_10..13_grad's products (the weights broadcast over it)
        float ga = gp[0] * pa[0], gb = gp[0] * pb[0], gc = gp[0] * pc[0], gd = gp[0] * pd[0];
        for (int c = 1; c < C; ++c) {
            const float gv = gp[c];
            ga = ga + gv * pa[c]; gb = gb + gv * pb[c]; gc = gc + gv * pc[c]; gd = gd + gv * pd[c];
        }
        generic_dtheta_pixel(t, ga, gb, gc, gd, Hi, Wi, s6);
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const float v = air_block_sum_256(s6[k], sh_red + 4 * k);
        if (tid == 0) d_theta_row[k] = v;
    }
}

__device__ __forceinline__ void transformer_nc_du(
    const float* __restrict__ theta, const float* __restrict__ d_out, float* __restrict__ d_U,
    int b, int c0, int ncg, int T, int Hi, int Wi, int C, int Ho, int Wo, int lds_ordered, float* sh_dU /* [ncg][NIp] */)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int NI = Hi * Wi, NIp = (NI + 3) & ~3, NO = Ho * Wo;
    for (int i = tid; i < ncg * NIp; i += THREADS) sh_dU[i] = 0.0f;
    float* dst = d_U + (size_t)b * NI * C + c0;
    for (int t = 0; t < T; ++t) {
        __syncthreads();
        if (wave < ncg) {
            const size_t row = (size_t)b * T + t;
            float th[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) th[k] = theta[row * 6 + k];
            const float* g = d_out + row * NO * C + c0 + wave;         // this wave's channel, stride C
            float* plane = sh_dU + wave * NIp;
            if (!lds_ordered) {
                // fallback for a part whose LDS atomics do not apply lanes in ascending order (lds_order_probe): ONE lane per
                // channel walks the terms -- slow, but the reference's scatter order by construction
                if (lane == 0)
                    for (int ph = 0; ph < 4; ++ph)
                        for (int p = 0; p < NO; ++p) {
                            const GenTap tp = generic_tap(th, p / Wo, p % Wo, Hi, Wi, Ho, Wo);
                            float wgt;
                            int idx;
                            generic_tap_term(tp, ph, Wi, wgt, idx);
                            plane[idx] = plane[idx] + wgt * g[(size_t)p * C];
                        }
            } else {
                // the gradient of the next 64 terms is loaded ahead of this instruction's adds (the index wraps into the next
                // tap's first pixels; past the last tap it re-reads them and the value is dropped)
                float gcur = lane < NO ? g[(size_t)lane * C] : 0.0f;
                for (int ph = 0; ph < 4; ++ph)
                    for (int p0 = 0; p0 < NO; p0 += 64) {
                        const int p = p0 + lane, pn = (p0 + 64 < NO ? p0 + 64 : 0) + lane;
                        const float gnext = pn < NO ? g[(size_t)pn * C] : 0.0f;
                        if (p < NO) {
                            const GenTap tp = generic_tap(th, p / Wo, p % Wo, Hi, Wi, Ho, Wo);
                            float wgt;
                            int idx;
                            generic_tap_term(tp, ph, Wi, wgt, idx);
                            lds_fadd(plane + idx, wgt * gcur);
                        }
                        gcur = gnext;
                    }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
        __syncthreads();
        // this transform's d U leaves the planes (and leaves them zero for the next one): a thread owns its elements of the
        // image's d U over all t, the sum over the rows runs in ascending t
        for (int i = tid; i < NI * ncg; i += THREADS) {
            const int p = i / ncg, k = i - p * ncg;
            float* src = sh_dU + k * NIp + p;
            const float v = *src;
            *src = 0.0f;
            float* d = dst + (size_t)p * C + k;
            *d = t == 0 ? v : *d + v;
        }
    }
}

__global__ __launch_bounds__(THREADS) void transformer_nc_bwd_kernel(
    const float* __restrict__ U, const float* __restrict__ theta, const float* __restrict__ d_out,
    float* __restrict__ d_U, float* __restrict__ d_theta, int T, int Hi, int Wi, int C, int Ho, int Wo,
    int cg, int ngroups, int lds_ordered)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    // per image: `ngroups` channel groups of d U (none without d_U), then the T rows of d theta (none without d_theta)
    const int per = ngroups + (d_theta ? T : 0);
    const int b = blockIdx.x / per, y = blockIdx.x - b * per;
    if (y < ngroups) {
        const int c0 = y * cg;
        transformer_nc_du(theta, d_out, d_U, b, c0, min(cg, C - c0), T, Hi, Wi, C, Ho, Wo, lds_ordered, smem + 32);
    } else {
        const size_t row = (size_t)b * T + (y - ngroups);
        transformer_nc_dtheta(U + (size_t)b * Hi * Wi * C, theta + row * 6, d_out + row * Ho * Wo * C, d_theta + row * 6,
                              Hi, Wi, C, Ho, Wo, smem);
    }
}

// ---------------------------------------------------------------------------
// write backward, EXACT adjoint (literal == 0, backward="exact": the fp64-gradient tests): gradient wrt the window
// (separable, gather form, degenerate taps merged -- their two weights cancel exactly in real arithmetic), wrt
// theta_recon -> (s,x,y), and wrt z_pres.  One workgroup per (image, time step): every step sees the same
// d loss / d canvas.
// ---------------------------------------------------------------------------
// 16 waves per workgroup: every phase is a latency chain, 4 waves per SIMD hide it
constexpr int WB_THREADS = 1024;

// ---- parts the three orders share ----------------------------------------------------------------------------------------
// agent-scope relaxed accesses of the words one workgroup hands to another inside a launch (global_ ... sc1: served by the
// memory side, never by a CU's L1)
typedef __attribute__((address_space(1))) float air_global_float;
typedef __attribute__((address_space(1))) int32_t air_global_int;
__device__ __forceinline__ void store_agent(float* p, float v) {
    __hip_atomic_store((air_global_float*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_agent(int32_t* p, int32_t v) {
    __hip_atomic_store((air_global_int*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float load_agent(const float* p) {
    return __hip_atomic_load((const air_global_float*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int32_t load_agent(const int32_t* p) {
    return __hip_atomic_load((const air_global_int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
struct LoadPlain { template <typename T> __device__ __forceinline__ T operator()(const T* p) const { return *p; } };
struct LoadAgent { template <typename T> __device__ __forceinline__ T operator()(const T* p) const { return load_agent(p); } };
// the batch means on one workgroup of NT threads: loss = mean(loss_item) :593,610; accuracy = mean(target == digits)
// :597-611 (air_finalize).  `ld` reads what the launch in front (plain) or another workgroup of this launch (agent scope)
// wrote.  sh_red is free again behind the caller's next barrier
template <int NT, typename Load>
__device__ __forceinline__ void batch_means(const air_write_bwd_t& a, float* sh_red, int tid, Load ld) {
    float r4[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < a.B; i += NT) {
        r4[0] += ld(a.fin_loss_item + i);
        r4[1] += (a.fin_targets[i] == ld(a.fin_digits + i)) ? 1.0f : 0.0f;
    }
    air_block_sum4<NT / 64>(r4, sh_red);
    if (tid == 0) { a.fin_scalars[0] = r4[0] / (float)a.B; a.fin_scalars[1] = r4[1] / (float)a.B; }
}
// where(active, ., 0): an inactive item has no gradient
template <int NT>
__device__ __forceinline__ void zero_item(float* dgen, unsigned short* dgen16, float* dsx, int ww, int tid) {
    for (int p = tid; p < ww; p += NT) { dgen[p] = 0.0f; if (dgen16) dgen16[p] = 0; }
    if (tid < 4) dsx[tid] = 0.0f;
}
// d loss / d canvas of an image into LDS, 8 loads in flight per thread per pass (one pass: 8 * NT elements from p0)
template <int NT>
__device__ __forceinline__ void stage_g_load(const float* gsrc, int CC, int tid, int p0, float (&r)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int p = p0 + k * NT + tid; r[k] = p < CC ? gsrc[p] : 0.0f; }
}
template <int NT>
__device__ __forceinline__ void stage_g_store(float* sh_g, int CC, int tid, int p0, const float (&r)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int p = p0 + k * NT + tid; if (p < CC) sh_g[p] = r[k]; }
}
template <int NT>
__device__ __forceinline__ void stage_g(const float* gsrc, float* sh_g, int CC, int tid, int from) {
    for (int p0 = from; p0 < CC; p0 += 8 * NT) {
        float r[8];
        stage_g_load<NT>(gsrc, CC, tid, p0, r);
        stage_g_store<NT>(sh_g, CC, tid, p0, r);
    }
}
// a window pixel's gradient wrt the pre-sigmoid input and its bf16 twin
__device__ __forceinline__ void store_dgen(float* dgen, unsigned short* dgen16, int it, float dgv) {
    dgen[it] = dgv;
    if (dgen16) dgen16[it] = air_bf16_of(dgv);
}

__global__ __launch_bounds__(WB_THREADS) void write_bwd_kernel(air_write_bwd_t a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    const int C = a.C, w = a.w;
    const size_t row = (size_t)t * a.B + b;
    AIR_STAMP(0);
    float* sh_red = smem;                                  // [64]
    Tap* sh_tx = reinterpret_cast<Tap*>(smem + 64);        // [C]
    Tap* sh_ty = sh_tx + C;                                // [C]
    float* sh_t = reinterpret_cast<float*>(sh_ty + C);     // [C] linspace
    int* sh_rng = reinterpret_cast<int*>(sh_t + C);        // [8*w]: per source index, the range of outputs whose taps hit it
    float* sh_win = reinterpret_cast<float*>(sh_rng + 8 * w);   // [w*w]
    float* sh_T = sh_win + w * w;                          // [C*w]
    float* sh_g = sh_T + C * w;                            // [C*C] d loss / d canvas of this image

    if (a.fin_scalars && b == 0 && t == 0) {
        batch_means<WB_THREADS>(a, sh_red, tid, LoadPlain{});
        __syncthreads();                                   // sh_red is reused below
    }
    const float* at = a.att + row * AIR_ATT_STRIDE;
    float* dgen = a.d_gen_pre + row * w * w;
    unsigned short* dgen16 = a.d_gen_pre16 ? a.d_gen_pre16 + row * w * w : nullptr;
    float* dsx = a.d_sxy_write + row * 4;
    if (at[AIR_ATT_MASK] == 0.0f) {
        zero_item<WB_THREADS>(dgen, dgen16, dsx, w * w, tid);
        return;
    }
    const float s = at[AIR_ATT_S], x = at[AIR_ATT_X], y = at[AIR_ATT_Y], z = at[AIR_ATT_Z];
    const float ia = 1.0f / s, bx = (-x) / s, by = (-y) / s;
    for (int j = tid; j < C; j += WB_THREADS) {
        float tv;
        sh_tx[j] = axis_tap(j, C, w, ia, bx, &tv);
        sh_ty[j] = axis_tap(j, C, w, ia, by);
        sh_t[j] = tv;
    }
    const float* v = a.vrec + row * w * w;
    for (int p = tid; p < w * w; p += WB_THREADS) sh_win[p] = v[p];
    // one coalesced pass with 8 loads in flight per thread; every later access is LDS
    stage_g<WB_THREADS>(a.d_recon + (size_t)b * C * C, sh_g, C * C, tid, 0);
    __syncthreads();
    // source index q is touched by a contiguous range of output coordinates (taps are monotone): one merged range
    // per index, degenerate (both taps clipped to one index) outputs skipped
    AIR_STAMP(1);
    if (tid < 2 * w) {
        const Tap* tp = (tid < w) ? sh_tx : sh_ty;
        const int q = (tid < w) ? tid : tid - w;
        int lo0 = C, hi0 = -1;
        for (int j = 0; j < C; ++j) {
            const Tap tt = tp[j];
            if (tt.i0 != tt.i1 && (tt.i0 == q || tt.i1 == q)) { lo0 = min(lo0, j); hi0 = max(hi0, j); }
        }
        int* r = sh_rng + (tid < w ? 0 : 4 * w) + 4 * q;
        r[0] = lo0; r[1] = hi0; r[2] = C; r[3] = -1;
    }
    __syncthreads();

    const float* g = sh_g;
    // stage 1: T[I][q] = sum_J g[I][J] * Rx[J][q]
    for (int it = tid; it < C * w; it += WB_THREADS) {
        const int I = it / w, q = it % w;
        float acc = 0.0f;
        for (int J = sh_rng[4 * q]; J <= sh_rng[4 * q + 1]; ++J) {
            const Tap tt = sh_tx[J];
            const float wq = (tt.i0 != tt.i1) ? ((tt.i0 == q ? tt.w0 : 0.0f) + (tt.i1 == q ? tt.w1 : 0.0f)) : 0.0f;
            acc += g[I * C + J] * wq;
        }
        sh_T[I * w + q] = acc;
    }
    AIR_STAMP(2);
    // theta / z gradients, per canvas pixel (independent of stage 1)
    const float half_w = ((float)w - 1.001f) / 2.0f;
    float da = 0.f, dbx = 0.f, dby = 0.f, dz = 0.f;
    const int di = WB_THREADS / C, dj = WB_THREADS % C;          // (i, j) advance per WB_THREADS pixels
    int i = tid / C, j = tid % C;
#pragma unroll 2
    for (int p = tid; p < C * C; p += WB_THREADS) {
        const Tap tx = sh_tx[j], ty = sh_ty[i];
        const float Ia = sh_win[ty.i0 * w + tx.i0], Ib = sh_win[ty.i1 * w + tx.i0];
        const float Ic = sh_win[ty.i0 * w + tx.i1], Id = sh_win[ty.i1 * w + tx.i1];
        const float gv = g[p];
        const int ci = i, cj = j;
        i += di; j += dj;
        if (j >= C) { j -= C; ++i; }
        // a degenerate axis (both taps clipped to one index) is exactly 0 in real arithmetic;
        // the fp32 residue the forward keeps there (~1e-7) would be multiplied by g ~ 1e9/B
        // (d log(r + 1e-9) at r ~ 0) and drown d z_pres in rounding noise.
        // (the reference's autodiff multiplies the residue by g like any other value: the graph-order kernels below)
        if (tx.i0 != tx.i1 && ty.i0 != ty.i1) dz += gv * bilinear4(tx, ty, Ia, Ib, Ic, Id);
        const float gz = gv * z;
        const float gX = gz * ((Ic - Ia) * ty.w0 + (Id - Ib) * ty.w1) * half_w;
        const float gY = gz * ((Ib - Ia) * tx.w0 + (Id - Ic) * tx.w1) * half_w;
        da += gX * sh_t[cj] + gY * sh_t[ci];
        dbx += gX;
        dby += gY;
    }
    AIR_STAMP(3);
    {
        float red4[4] = {da, dbx, dby, dz};
        air_block_sum4<WB_THREADS / 64>(red4, sh_red);   // contains the __syncthreads() that publishes sh_T
        da = red4[0]; dbx = red4[1]; dby = red4[2]; dz = red4[3];
    }
    if (tid == 0) {
        // a = 1/s, bx = -x/s, by = -y/s
        const float is2 = 1.0f / (s * s);
        dsx[0] = (-da + dbx * x + dby * y) * is2;
        dsx[1] = -dbx / s;
        dsx[2] = -dby / s;
        dsx[3] = dz;
    }
    AIR_STAMP(4);
    // stage 2: dU[p][q] = z * sum_I Ry[I][p] * T[I][q]; fold the sigmoid of vae.py:39-41
    for (int it = tid; it < w * w; it += WB_THREADS) {
        const int p = it / w, q = it % w;
        const int* ry = sh_rng + 4 * w + 4 * p;
        float acc = 0.0f;
        for (int I = ry[0]; I <= ry[1]; ++I) {
            const Tap tt = sh_ty[I];
            const float wp = (tt.i0 != tt.i1) ? ((tt.i0 == p ? tt.w0 : 0.0f) + (tt.i1 == p ? tt.w1 : 0.0f)) : 0.0f;
            acc += sh_T[I * w + q] * wp;
        }
        const float du = z * acc;
        const float r = sh_win[it];
        store_dgen(dgen, dgen16, it, du * (r * (1.0f - r)));   // (the exact adjoint's own grouping; the graph orders: wb_store_slot)
    }
    AIR_STAMP(6);
}


// ---------------------------------------------------------------------------
// write backward in the op order of the reference's SAVED graph (literal == 2; the default
// backward="reference" of AIRModel).  What the graph does with d loss / d window_recon
// (model/air-model.meta, executed node by node by the graph executor of tests/test_graph_exec.py):
//   * the four Gather gradients (taps a=(y0,x0), b=(y1,x0), c=(y0,x1), d=(y1,x1)) are CONCATENATED and
//     reduced by ONE UnsortedSegmentSum: every window pixel ("slot") is a single fp32 accumulator
//     that receives its a-terms in canvas-pixel order, then its b-, c- and d-terms.  The terms of an
//     out-of-range canvas pixel cancel exactly in real arithmetic (both taps clip to one border
//     index), but not in this accumulation order: the border slots keep a rounding residue of
//     ~ulp(sum of |terms|), which at unexplained ink (d log(r + 1e-9) ~ 1e9/B) is orders of magnitude
//     above the exact gradient -- that residue is part of the reference's training signal
//     (tests/golden/graph_b64.npz: |g| 1.6e6 in fp32 vs 1.1e3 in fp64 at initialisation).
//   * per canvas pixel, the gradients wrt the sampling coordinates are summed by AddN_10 / AddN_11 in
//     the order wa, wb, wc, wd (graph_dxy).
// Reproduced here bit for bit (tests/test_gpu_graph_golden.py) and deterministically:
//   stage T: all threads compute term = (wx*wy) * (z*g) of every tap of every canvas pixel and store it
//            in a "rectangle-blocked" layout: taps are monotone, so the pixels of one slot form a
//            rectangle (row run x column run) and each slot's terms of a tap are one contiguous
//            stream in exactly the accumulation order;
//   stage C: one lane per slot streams its four runs through a single fp32 register accumulator
//            (a lone wave issues a dependent v_add_f32 every ~8 cycles -- fine for the short
//            in-range and edge runs).  The FOUR CORNER slots own every pixel that is outside the
//            glimpse in both axes -- (C - s*C)^2 terms per tap, most of the canvas -- and go through
//            the LDS instead: after everything else is published, waves 0..3 feed one corner each, 64 terms per
//            instruction, to ds_add_f32 on one LDS word per corner.  gfx950's LDS applies the lanes of one
//            instruction in ascending lane order and a wave's instructions in program order
//            (measured: tools/exp/lds_atomic_order.hip; pinned by the bit-for-bit test), i.e. it IS
//            a sequential fp32 accumulator, at ~4 cycles per term and without occupying the VALU.  While it runs,
//            every other LDS request of the CU starves, so the short chains go first and the coordinate-gradient
//            pixel loop -- rewritten to touch no LDS at all -- runs on the other twelve waves underneath it.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float stream_add(float acc, const float* T, int start, int n) {
    int k = start;
    const int end = start + n;
    while (k < end && (k & 3)) { acc += T[k]; ++k; }
    const int nb = (end - k) >> 2;
    if (nb > 0) {
        // two 16-byte LDS reads in flight ahead of the dependent adds; the look-ahead index is clamped
        // (a harmless re-read) so that every access stays an LDS access of this stream
        const float4* p4 = reinterpret_cast<const float4*>(T + k);
        float4 c0 = p4[0], c1 = p4[min(1, nb - 1)];
        for (int b = 0; b < nb; ++b) {
            const float4 nx = p4[min(b + 2, nb - 1)];
            acc += c0.x; acc += c0.y; acc += c0.z; acc += c0.w;
            c0 = c1; c1 = nx;
        }
        k += nb * 4;
    }
    while (k < end) { acc += T[k]; ++k; }
    return acc;
}

// ALLPH: the terms of all four taps are resident (4*C*C floats of LDS, no barrier between taps);
// otherwise one tap at a time through one buffer (large canvases)
// CARRIED (literal == 4, backward="reference_carried"): the same term streams -- per window pixel the a-, b-, c-, d-tap
// terms in canvas-pixel order -- with every (slot, tap) stream of n terms cut into at most WB_CHUNKS contiguous chunks of
// max(ceil(n / WB_CHUNKS), WB_CHUNK_MIN) terms that are walked side by side on register chains.  A stream of up to 64 terms
// is ONE chunk, so only the border slots that collect the out-of-range pixels are cut at all.  No LDS atomics, no lane-order
// property, no probe; the coordinate / z gradients are taken in the term pass.
// (Round 5 also shipped the plain chunked form -- every chunk from +0.0, the chunk sums added left to right, "blocked16":
// 13.4 us against 17.7, and 4 of 24 training runs stuck on a count class.  Removed)
//   * a slot whose four streams all fit one chunk (<= 64 terms each: every slot but the corners and a few long borders) is
//     summed exactly as the reference sums it -- one accumulator through its a-, b-, c-, d-terms;
//   * a slot with a longer stream walks every chunk TWICE: C_k = chunk k from +0.0, Q_k = chunk k from P_k, with P_k the
//     running sum of the C's before it (a deterministic stand-in for the reference's accumulator at the chunk's start);
//     the slot's sum is Q_last + sum_{k < last} (Q_k - P_k+1), the corrections added left to right: Q_k and P_k+1 are two
//     roundings of the same real number, their difference is a few ulps and exact.  Every add of the Q chains rounds at
//     the magnitude it rounds at in the reference's one long chain and nothing else rounds at that magnitude, so the
//     cancellation residue the out-of-range terms leave keeps its size (mean |error| 1.0x the sequential order's over 2116
//     corner streams) -- DESIGN.md section 10.
//   Two chains of n / 16 adds per corner instead of one of 4 n; no LDS atomics, no probe.
constexpr int WB_CHUNKS = 16, WB_CHUNK_MIN = 64;
__device__ __forceinline__ int wb_chunk_len(int n) { return max((n + WB_CHUNKS - 1) / WB_CHUNKS, WB_CHUNK_MIN); }
// c += every term, q += every term: the two chains of one chunk in ONE pass over its terms (independent: they overlap)
__device__ __forceinline__ void stream_add2(float& c, float& q, const float* T, int start, int n) {
    int k = start;
    const int end = start + n;
    while (k < end && (k & 3)) { const float t = T[k]; c += t; q += t; ++k; }
    const int nb = (end - k) >> 2;
    if (nb > 0) {
        const float4* p4 = reinterpret_cast<const float4*>(T + k);
        float4 c0 = p4[0], c1 = p4[min(1, nb - 1)];
        for (int b = 0; b < nb; ++b) {
            const float4 nx = p4[min(b + 2, nb - 1)];
            c += c0.x; q += c0.x; c += c0.y; q += c0.y; c += c0.z; q += c0.z; c += c0.w; q += c0.w;
            c0 = c1; c1 = nx;
        }
        k += nb * 4;
    }
    while (k < end) { const float t = T[k]; c += t; q += t; ++k; }
}
// ---------------------------------------------------------------------------
// The graph-order and the carried write backward as parts: every phase is ONE free function that
// takes what it uses, and the four bodies at the end -- graph all-taps (with or without the compose fold in front), graph
// one-tap, carried all-taps, carried one-tap -- are linear sequences of them with their barriers in sight.
// ---------------------------------------------------------------------------
static_assert(WB_THREADS == CF_THREADS, "the compose fold runs compose's parts on the write backward's workgroup");
constexpr int WB_NW = WB_THREADS / 64;
// waves 0..3 feed one corner each to the atomic pipe; the pixel loop runs beside them on the other twelve
constexpr int WB_TH0 = 4 * 64, WB_THN = WB_THREADS - WB_TH0;

// what a workgroup knows about itself and its item, built once: the LDS views (write_bwd_graph_layout), the sizes, the
// thread's place, the item's record and the output pointers
struct WbCtx {
    float* sh_red; float* sh_acc; int* sh_cn;    // WbLayout's red, acc, and the counts behind the four accumulators
    Tap* sh_tx; Tap* sh_ty; float* sh_t; int4* sh_ci; int4* sh_ri; int* sh_run; float* sh_win;
    // d loss / d (masked z * window_recon): staged in LDS when all taps are resident (small canvases); a large canvas
    // reads it from memory where needed (its 5 uses per pixel hit L2: every step of an image reads the same row) --
    // 76 KB instead of 140 KB of LDS at 128x128.  (Two workgroups per CU do NOT follow from that: the <false> instances
    // hold 110 and 64 VGPRs, i.e. 4 and 7 waves per SIMD, and a second 16-wave workgroup needs 8.  DESIGN.md section 32,
    // open items.)
    float* sh_g; float* sh_T;
    int C, w, CC, CCp, tid, lane, wave;
    int lin, b, t;           // linear workgroup id; the item
    const float* at; const float* gsrc; const float* v;
    float* dgen; unsigned short* dgen16; float* dsx;
    float s, x, y, z, ia, bx, by;
};
// which (image, step) item this workgroup computes: its grid position, or -- a.order given -- entry `linear block id` of
// the longest-first permutation the compose launch left (wb_order_block)
template <bool ALLPH>
__device__ __forceinline__ WbCtx wb_ctx(const air_write_bwd_t& a, float* smem) {
    WbCtx k;
    k.lin = (int)(blockIdx.y * gridDim.x + blockIdx.x);
    const int item = a.order ? a.order[k.lin] : k.lin;
    k.b = item % a.B; k.t = item / a.B;
    k.tid = threadIdx.x; k.lane = k.tid & 63; k.wave = k.tid >> 6;
    k.C = a.C; k.w = a.w; k.CC = k.C * k.C; k.CCp = (k.CC + 3) & ~3;
    const WbLayout L = write_bwd_graph_layout(k.C, k.w, ALLPH);
    k.sh_red = smem + L.red; k.sh_acc = smem + L.acc; k.sh_cn = reinterpret_cast<int*>(k.sh_acc) + 4;
    k.sh_tx = reinterpret_cast<Tap*>(smem + L.tx); k.sh_ty = reinterpret_cast<Tap*>(smem + L.ty); k.sh_t = smem + L.t;
    k.sh_ci = reinterpret_cast<int4*>(smem + L.ci); k.sh_ri = reinterpret_cast<int4*>(smem + L.ri);
    k.sh_run = reinterpret_cast<int*>(smem + L.run); k.sh_win = smem + L.win; k.sh_g = smem + L.g; k.sh_T = smem + L.T;
    const size_t row = (size_t)k.t * a.B + k.b;
    k.at = a.att + row * AIR_ATT_STRIDE; k.gsrc = a.d_recon + (size_t)k.b * k.CC; k.v = a.vrec + row * k.w * k.w;
    k.dgen = a.d_gen_pre + row * k.w * k.w; k.dgen16 = a.d_gen_pre16 ? a.d_gen_pre16 + row * k.w * k.w : nullptr;
    k.dsx = a.d_sxy_write + row * 4;
    k.s = k.x = k.y = k.z = k.ia = k.bx = k.by = 0.0f;
    return k;
}
// theta_recon = [[1/s, 0, -x/s], [0, 1/s, -y/s]] (air_model.py:353-356) of the item
__device__ __forceinline__ void wb_item(WbCtx& k, float s, float x, float y, float z) {
    k.s = s; k.x = x; k.y = y; k.z = z;
    k.ia = 1.0f / s; k.bx = (-x) / s; k.by = (-y) / s;
}
// the per-thread coordinate / z gradient sums
struct WbGrad { float d00, d02, d11, d12, dz; };

// corner index -> the corner slot's window row p and column q
__device__ __forceinline__ void corner_pq(int c, int w, int& p, int& q) { p = (c & 2) ? w - 1 : 0; q = (c & 1) ? w - 1 : 0; }
// start / length of slot (p, q)'s stream of tap ph
template <bool ALLPH>
__device__ __forceinline__ void slot_run(const WbCtx& k, int ph, int p, int q, int& start, int& n) {
    const int w = k.w, xa = ph >> 1, ya = 2 + (ph & 1);
    const int clo = k.sh_run[(xa * w + q) * 2], ncols = k.sh_run[(xa * w + q) * 2 + 1] - clo + 1;
    const int rlo = k.sh_run[(ya * w + p) * 2], nrows = k.sh_run[(ya * w + p) * 2 + 1] - rlo + 1;
    start = (ALLPH ? ph * k.CCp : 0) + rlo * k.C + nrows * clo;
    n = nrows * ncols;
}
// tap ph = a, b, c, d <-> (y0,x0), (y1,x0), (y0,x1), (y1,x1): its weight wa..wd (transformer.py:108-115) ...
__device__ __forceinline__ float wb_tap_weight(const Tap& tx, const Tap& ty, int ph) {
    return ((ph >> 1) ? tx.w1 : tx.w0) * ((ph & 1) ? ty.w1 : ty.w0);
}
// ... and where canvas pixel (i, j)'s term of tap ph lies in the tap's rectangle-blocked buffer: taps are monotone, so the
// pixels of one slot form a rectangle (row run x column run) and the slot's terms are one contiguous stream in exactly the
// accumulation order.  ci / ri: the run records of column j / row i
__device__ __forceinline__ int wb_term_pos(const int4& ci, const int4& ri, int i, int j, int C, int ph) {
    const bool x1 = ph >> 1, y1 = ph & 1;
    const int clo = x1 ? ci.z : ci.x, ncols = x1 ? ci.w : ci.y, rlo = y1 ? ri.z : ri.x, nrows = y1 ? ri.w : ri.y;
    return rlo * C + nrows * clo + (i - rlo) * ncols + (j - clo);
}
// SigmoidGrad of vae.py:39-41 on a slot's sum: dy * y * (1 - y), in the graph's order
__device__ __forceinline__ void wb_store_slot(const WbCtx& k, int it, float du) {
    const float r = k.sh_win[it];
    store_dgen(k.dgen, k.dgen16, it, (du * r) * (1.0f - r));
}

// ---- set-up -------------------------------------------------------------------------------------------------------------
// taps, linspace, empty runs, zeroed accumulators and partial rows, the window
__device__ __forceinline__ void wb_stage_tables(const WbCtx& k, float win_pre) {
    const int tid = k.tid, C = k.C, w = k.w;
    for (int j = tid; j < C; j += WB_THREADS) {
        float tv;
        k.sh_tx[j] = axis_tap(j, C, w, k.ia, k.bx, &tv);
        k.sh_ty[j] = axis_tap(j, C, w, k.ia, k.by);
        k.sh_t[j] = tv;
    }
    for (int it = tid; it < 4 * w; it += WB_THREADS) { k.sh_run[2 * it] = 0; k.sh_run[2 * it + 1] = -1; }
    if (tid < 8) k.sh_acc[tid] = 0.0f;
    if (tid >= 64 && tid < 64 + WB_NW * 8) k.sh_red[tid - 64] = 0.0f;          // the feeding waves publish no pixel-loop partials
    if (tid < w * w) k.sh_win[tid] = win_pre;
}
// every key (tap index) owns ONE contiguous run of canvas columns / rows (taps are monotone)
__device__ __forceinline__ void wb_key_runs(const WbCtx& k) {
    const int C = k.C, w = k.w;
    for (int it = k.tid; it < 4 * C; it += WB_THREADS) {
        const int arr = it / C, J = it % C;                 // arr: x0, x1, y0, y1
        const Tap* tp = (arr < 2) ? k.sh_tx : k.sh_ty;
        const int key = (arr & 1) ? tp[J].i1 : tp[J].i0;
        const int kp = J > 0 ? ((arr & 1) ? tp[J - 1].i1 : tp[J - 1].i0) : -1;
        const int kn = J < C - 1 ? ((arr & 1) ? tp[J + 1].i1 : tp[J + 1].i0) : -1;
        if (kp != key) k.sh_run[(arr * w + key) * 2] = J;
        if (kn != key) k.sh_run[(arr * w + key) * 2 + 1] = J;
    }
}
// ... and every canvas column / row the runs of its two keys: the term phase then needs ONE LDS round trip per
// pixel (two taps + two run records, all independent) instead of eight run lookups that wait for the taps
__device__ __forceinline__ void wb_run_records(const WbCtx& k) {
    const int C = k.C, w = k.w;
    for (int it = k.tid; it < 2 * C; it += WB_THREADS) {
        const int ax = it / C, J = it - ax * C;
        const Tap tp = ax ? k.sh_ty[J] : k.sh_tx[J];
        const int* r0 = k.sh_run + ((2 * ax) * w + tp.i0) * 2;
        const int* r1 = k.sh_run + ((2 * ax + 1) * w + tp.i1) * 2;
        (ax ? k.sh_ri : k.sh_ci)[J] = make_int4(r0[0], r0[1] - r0[0] + 1, r1[0], r1[1] - r1[0] + 1);
    }
}
// terms of corner slot c over its four taps
__device__ __forceinline__ void wb_corner_counts(const WbCtx& k) {
    const int w = k.w;
    if (k.tid < 4) {
        int tot = 0, pp, q;
        corner_pq(k.tid, w, pp, q);
        for (int ph = 0; ph < 4; ++ph) {
            const int xa = ph >> 1, ya = 2 + (ph & 1);
            const int ncols = k.sh_run[(xa * w + q) * 2 + 1] - k.sh_run[(xa * w + q) * 2] + 1;
            const int nrows = k.sh_run[(ya * w + pp) * 2 + 1] - k.sh_run[(ya * w + pp) * 2] + 1;
            tot += max(nrows, 0) * max(ncols, 0);
        }
        k.sh_cn[k.tid] = tot;
    }
}
// the shared set-up behind the mask test.  STAGE_G: d loss / d canvas into sh_g, its first pass from the registers the loads
// went out to before the mask test (the compose fold has filled sh_g itself; a large canvas does not stage it)
template <bool STAGE_G>
__device__ __forceinline__ void wb_setup(const WbCtx& k, float win_pre, const float (&g_pre)[8]) {
    wb_stage_tables(k, win_pre);
    if (STAGE_G) {
        stage_g_store<WB_THREADS>(k.sh_g, k.CC, k.tid, 0, g_pre);
        stage_g<WB_THREADS>(k.gsrc, k.sh_g, k.CC, k.tid, 8 * WB_THREADS);
    }
    __syncthreads();
    AIR_STAMP(41);
    wb_key_runs(k);
    __syncthreads();
    wb_run_records(k);
    wb_corner_counts(k);
    __syncthreads();
    AIR_STAMP(42);
}
// the front of the forms without the compose fold: the batch means on one workgroup of the launch (ordered: the lightest
// item's), the loads that do not depend on the record, the mask test.  false: the item is inactive and finished
template <bool ALLPH>
__device__ __forceinline__ bool wb_open(const air_write_bwd_t& a, WbCtx& k, float& win_pre, float (&g_pre)[8]) {
    if (a.fin_scalars && k.lin == (a.order ? (int)(gridDim.x * gridDim.y) - 1 : 0)) {
        batch_means<WB_THREADS>(a, k.sh_red, k.tid, LoadPlain{});
        __syncthreads();
    }
    AIR_STAMP(40);
    AIR_STAMP_WG(0);
    // the window and (small canvases) the first pass over d_recon do not depend on the record: their loads go out
    // BEFORE the mask test waits for it -- one memory round trip for the set-up instead of two
    win_pre = k.tid < k.w * k.w ? k.v[k.tid] : 0.0f;              // (w * w <= WB_THREADS: checked by the launcher)
    if (ALLPH) stage_g_load<WB_THREADS>(k.gsrc, k.CC, k.tid, 0, g_pre);
    if (k.at[AIR_ATT_MASK] == 0.0f) {                          // Select(active, ., 0): no gradient
        zero_item<WB_THREADS>(k.dgen, k.dgen16, k.dsx, k.w * k.w, k.tid);
        return false;
    }
    wb_item(k, k.at[AIR_ATT_S], k.at[AIR_ATT_X], k.at[AIR_ATT_Y], k.at[AIR_ATT_Z]);
    return true;
}

// ---- the compose fold (air_write_fwd_bwd; graph all-taps only): the compose pass runs at the front of this launch.  Every
// workgroup of image b builds d loss / d canvas of that image itself, straight into sh_g -- compose's tap tables and windows
// lie over sh_T, which nothing writes before the term phase -- and the workgroup of step 0 owns the image's forward outputs
// (write_fwd_kernel's, in its summation orders).  The batch means need every image's loss_item / run_digits: the owners
// count themselves on *arrive and the one that arrives last computes them (fold_signal / fold_means below).
// The lane that counts an owner workgroup on *arrive for all that workgroup's stores (the first lane of the last wave: that
// wave runs the pixel loop, not a corner feed), and the LDS word through which it tells the workgroup whether its add came
// last (a free word of the last wave's partials row: zeroed with the row, read behind a barrier)
constexpr int WB_SIG = WB_THREADS - 64;
__device__ __forceinline__ int* fold_last_word(const WbCtx& k) { return reinterpret_cast<int*>(k.sh_red) + (WB_NW - 1) * 8 + 7; }
// hand-off, producer side: the signalling lane stored the workgroup's two words (store_agent, fold_front); once those
// stores have completed it counts the workgroup with ONE returning agent-scope add
__device__ __forceinline__ int fold_signal(int32_t* arrive, int tid) {
    int ticket = -1;
    if (tid == WB_SIG) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ticket = __hip_atomic_fetch_add((air_global_int*)arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return ticket;
}
// hand-off, consumer side.  `last` is workgroup-uniform and was read from the word of fold_last_word behind a barrier the
// adding wave joined after its add had returned B - 1: every owner's words are complete.  The loop and the reduction of the
// two-launch form (batch_means), on agent-scope loads
__device__ __forceinline__ void fold_means(const air_write_bwd_t& a, int32_t* arrive, const WbCtx& k, bool last) {
    if (!last) return;
    batch_means<WB_THREADS>(a, k.sh_red, k.tid, LoadAgent{});
    if (k.tid == 0) store_agent(arrive, 0);                  // every owner has arrived: the next launch counts from 0
}
// The front itself.  false: the item is inactive and finished (an owner has then counted itself and, if last, run the means)
__device__ __forceinline__ bool fold_front(const air_write_bwd_t& a, const air_write_fwd_t& f, int32_t* arrive, WbCtx& k, bool owner,
                                           float& win_pre) {
    const int N = a.N, B = a.B, C = k.C, w = k.w, tid = k.tid, b = k.b;
    // compose's scratch in write_fwd_kernel's layout (write_smem), over the term buffer; behind it the two words run_loss,
    // run_digits for the signalling lane
    const ComposeLds L = compose_lds(k.sh_T, N, C, w);
    float* c_sig = L.win + (size_t)N * w * w;
    const size_t base = (size_t)b * k.CC;
    // ONE memory round trip for the set-up: this item's record, the image row and the first WPRE * WB_THREADS window
    // elements go out before anything waits (the tap tables wait for the records of all steps; what is behind the
    // prefetched window elements is loaded after them)
    const float mask_own = k.at[AIR_ATT_MASK];
    wb_item(k, k.at[AIR_ATT_S], k.at[AIR_ATT_X], k.at[AIR_ATT_Y], k.at[AIR_ATT_Z]);
    constexpr int WPRE = 4;
    float xs[COMPOSE_XPRE], wpre[WPRE];
    const bool xpre = compose_prefetch_image(f.images, base, k.CC, tid, xs);
#pragma unroll
    for (int q = 0; q < WPRE; ++q) {
        const int it = tid + q * WB_THREADS;
        wpre[q] = compose_window_at(a.vrec, b, B, w, it < N * w * w ? it : 0);
    }
    if (owner) compose_vae_kl<WB_NW>(f.ml, f.dyn, b, B, N, f.Z, k.lane, k.wave, L.kl);
    compose_stage_taps(a.att, b, B, N, C, w, tid, WB_THREADS, L.tx, L.ty);
#pragma unroll
    for (int q = 0; q < WPRE; ++q) { const int it = tid + q * WB_THREADS; if (it < N * w * w) L.win[it] = wpre[q]; }
    compose_stage_windows(a.vrec, b, B, N, w, tid + WPRE * WB_THREADS, WB_THREADS, L.win);
    compose_fetch_records(a.att, b, B, N, tid, L);
    __syncthreads();
    if (!owner && mask_own == 0.0f) {                    // Select(active, ., 0): no gradient, and not this image's owner
        zero_item<WB_THREADS>(k.dgen, k.dgen16, k.dsx, w * w, tid);
        return false;
    }
    if (owner && tid == 0) {
        float loss;
        int digits;
        compose_running_loss(L, f.att, b, B, N, loss, digits);
        f.run_loss[b] = loss;
        c_sig[0] = loss;
        c_sig[1] = __builtin_bit_cast(float, digits);
    }
    // canvas + Bernoulli cross-entropy, pixel by pixel: d loss / d canvas into sh_g; the owner also stores it and the
    // clipped reconstruction and sums the cross-entropy
    float acc = compose_pixels<2, true>(L, f.images, base, xs, xpre, N, C, w, f.dyn[AIR_DYN_GRAD_SCALE], tid, owner,
                                        f.recon, f.d_recon, k.sh_g);
    if (owner) {
        acc = air_block_sum_n<WB_NW>(acc, L.red);
        const float rl = -acc;
        if (tid == 0) f.rec_loss[b] = rl;
        if (tid == WB_SIG) {
            store_agent(f.loss_item + b, c_sig[0] + rl);            // loss += reconstruction_loss :593
            store_agent(f.run_digits + b, __builtin_bit_cast(int, c_sig[1]));
        }
    }
    AIR_STAMP_WG(7);
    if (mask_own == 0.0f) {                              // (an owner only) no gradient: count the workgroup and finish here
        zero_item<WB_THREADS>(k.dgen, k.dgen16, k.dsx, w * w, tid);
        const int ticket = fold_signal(arrive, tid);
        int* sh_last = fold_last_word(k);
        if (tid == WB_SIG) *sh_last = ticket == a.B - 1 ? 1 : 0;
        __syncthreads();
        fold_means(a, arrive, k, *sh_last != 0);
        return false;
    }
    win_pre = tid < w * w ? L.win[(size_t)k.t * w * w + tid] : 0.0f;
    return true;
}

// ---- terms --------------------------------------------------------------------------------------------------------------
// stage T: term = (wx*wy) * (z*g) of taps PH0 .. PH1-1 of every canvas pixel into the rectangle-blocked buffers.  One tap
// per pass (large canvases): the tap is a compile-time constant of the term loop (its six operand selects fold away)
template <bool ALLPH, int PH0, int PH1>
__device__ __forceinline__ void stage_terms(const WbCtx& k) {
    const int C = k.C, di = WB_THREADS / C, dj = WB_THREADS % C;
    int i = k.tid / C, j = k.tid % C;
    for (int p = k.tid; p < k.CC; p += WB_THREADS) {
        const Tap tx = k.sh_tx[j], ty = k.sh_ty[i];
        const float gp = k.z * (ALLPH ? k.sh_g[p] : k.gsrc[p]);                    // canvas/mul_grad: z * Select_grad
        const int4 ci = k.sh_ci[j], ri = k.sh_ri[i];
#pragma unroll
        for (int ph = PH0; ph < PH1; ++ph)
            k.sh_T[(ALLPH ? ph * k.CCp : 0) + wb_term_pos(ci, ri, i, j, C, ph)] = wb_tap_weight(tx, ty, ph) * gp;
        i += di; j += dj;
        if (j >= C) { j -= C; ++i; }
    }
}
// CARRIED: the terms of taps PH0 .. PH1-1 (and, THETA, the theta / z gradients, taken where the pixel's taps and
// d_recon are in registers anyway: the window from LDS -- nothing starves the LDS in this mode).  A thread owns ONE
// canvas column j and the rows i0, i0 + RPP, ...: the column's tap, its runs and its linspace value are loop
// invariants, the row's are wave-wide broadcasts.  Per-thread sums over a fixed pixel set, combined over the waves in a
// fixed order at the end.  A row outside the glimpse (both y taps clipped to one index: ty.w1 == -ty.w0, Ia == Ib,
// Ic == Id) contributes EXACT zeros to all five sums -- the a / b and c / d legs of AddN_10 / AddN_11 and of the
// bilinear sum cancel pairwise before anything rounds -- and is skipped; an out-of-range COLUMN does not cancel
// exactly (that is the x residue) and is not.
template <bool ALLPH, int PH0, int PH1, bool THETA>
__device__ __forceinline__ void carried_terms(const WbCtx& k, WbGrad& G) {
    const int C = k.C, w = k.w;
    const int RPP = WB_THREADS / C, bj = k.tid % C, bi0 = k.tid / C;
    if (bi0 >= RPP) return;
    const Tap tx = k.sh_tx[bj];
    const int4 ci = k.sh_ci[bj];
    const float tjv = k.sh_t[bj];
    const float cw = (float)w - 1.001f;
    for (int i = bi0; i < C; i += RPP) {
        const Tap ty = k.sh_ty[i];
        const int4 ri = k.sh_ri[i];
        const float g0 = ALLPH ? k.sh_g[i * C + bj] : k.gsrc[i * C + bj];
        const float gp = k.z * g0;                                              // canvas/mul_grad: z * Select_grad
        float wq[4];
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) wq[ph] = wb_tap_weight(tx, ty, ph);
#pragma unroll
        for (int ph = PH0; ph < PH1; ++ph)
            k.sh_T[(ALLPH ? ph * k.CCp : 0) + wb_term_pos(ci, ri, i, bj, C, ph)] = wq[ph] * gp;
        if (THETA && ty.i0 != ty.i1) {
            const float Ia = k.sh_win[ty.i0 * w + tx.i0], Ib = k.sh_win[ty.i1 * w + tx.i0];
            const float Ic = k.sh_win[ty.i0 * w + tx.i1], Id = k.sh_win[ty.i1 * w + tx.i1];
            G.dz += g0 * (((wq[0] * Ia + wq[1] * Ib) + wq[2] * Ic) + wq[3] * Id);   // canvas/mul_grad: Select_grad * window_recon
            float gX, gY;
            graph_dxy(gp, Ia, Ib, Ic, Id, tx, ty, cw, gX, gY);
            G.d00 += gX * tjv; G.d02 += gX;                                     // MatMul_grad: rows of theta x (x_t, y_t, 1)
            G.d11 += gY * k.sh_t[i]; G.d12 += gY;
        }
    }
}
// a wave's coordinate / z gradient partials (combined over the waves in a fixed order at the end: finish_theta)
__device__ __forceinline__ void publish_wave_partials(const WbCtx& k, WbGrad& G) {
    G.d00 = air_wave_sum(G.d00); G.d02 = air_wave_sum(G.d02); G.d11 = air_wave_sum(G.d11); G.d12 = air_wave_sum(G.d12);
    G.dz = air_wave_sum(G.dz);
    if (k.lane == 0) { float* r = k.sh_red + k.wave * 8; r[0] = G.d00; r[1] = G.d02; r[2] = G.d11; r[3] = G.d12; r[4] = G.dz; }
}

// ---- slots --------------------------------------------------------------------------------------------------------------
// which window pixel ("slot") a thread accumulates.  CARRIED: waves 0..3 take the corner slots' chunks, so the other
// slots start at thread 256 and whatever does not fit behind it falls to the first threads (after their corner work);
// the 4 (w - 2) border slots -- the only other long streams: a row or a column of out-of-range pixels each -- come
// first, packed into the same waves, the interior slots (a handful of terms per tap) fill the rest
struct WbSlot { int sl, sp, sq; bool is_slot, corner; };
template <bool CARRIED>
__device__ __forceinline__ WbSlot wb_slot(const WbCtx& k, bool lds_ordered, bool ring_ok) {
    const int tid = k.tid, w = k.w;
    WbSlot s;
    s.sl = tid; s.sp = tid / w; s.sq = tid % w;
    s.is_slot = tid < w * w;
    if (CARRIED) {
        const int u = tid >= 4 * 64 ? tid - 4 * 64 : tid + (WB_THREADS - 4 * 64);
        const int wm = max(w - 2, 1), ne = 4 * (w - 2);
        s.is_slot = u < w * w - 4;
        if (u < ne) {
            const int side = u / wm, r = u - side * wm + 1;
            s.sp = side == 0 ? 0 : side == 1 ? w - 1 : r;
            s.sq = side < 2 ? r : (side == 2 ? 0 : w - 1);
        } else {
            const int v = u - ne, vr = v / wm;
            s.sp = 1 + vr; s.sq = 1 + (v - vr * wm);
        }
        s.sl = s.sp * w + s.sq;
    }
    // (a part whose LDS atomics are not lane-ordered -- lds_order_probe -- has no "corner" slots: their four long runs go
    // through the register chains like every other slot's; slow, but the same sequential order by construction)
    s.corner = !CARRIED && (lds_ordered || ring_ok) && s.is_slot && (s.sp == 0 || s.sp == w - 1) && (s.sq == 0 || s.sq == w - 1);
    return s;
}
// stage C: one lane per slot streams its runs of taps ph0 .. ph1-1 through a single fp32 register accumulator
template <bool ALLPH>
__device__ __forceinline__ void chains(const WbCtx& k, const WbSlot& s, int ph0, int ph1, float& acc) {
    if (s.is_slot && !s.corner)
        for (int ph = ph0; ph < ph1; ++ph) {
            int start, n;
            slot_run<ALLPH>(k, ph, s.sp, s.sq, start, n);
            acc = stream_add(acc, k.sh_T, start, n);
        }
}
// the non-corner slots' outputs
__device__ __forceinline__ void publish(const WbCtx& k, const WbSlot& s, float acc) {
    if (s.is_slot && !s.corner) wb_store_slot(k, s.sl, acc);
}
__device__ __forceinline__ void publish_corner(const WbCtx& k, int c, float du) {
    int p, q;
    corner_pq(c, k.w, p, q);
    wb_store_slot(k, p * k.w + q, du);
}

// ---- corners, graph order -------------------------------------------------------------------------------------------------
// The corner slots' streams -> ds_add_f32 on one LDS word per corner: wave c feeds corner c, 64
// consecutive terms per instruction, tap after tap (an instruction costs ~140 + 1.8 cycles per active
// lane, tools/exp/lds_atomic_cost.hip).  16 instructions per batch; reads, adds and waits are inline asm
// (the compiler's own s_waitcnt bookkeeping would put an lgkmcnt(0) in front of every add).
template <bool ALLPH>
__device__ __forceinline__ void feed_corner(const WbCtx& ctx, int c, int ph0, int ph1) {
    const int lane = ctx.lane, w = ctx.w;
    float* const sh_T = ctx.sh_T;
    float* const sh_acc = ctx.sh_acc;
    constexpr int NB = 16;
    // stream descriptors of this corner: lane ph computes tap ph's run, broadcast to scalars
    int my_start = 0, my_n = 0;
    if (lane < 4) slot_run<ALLPH>(ctx, lane, (c & 2) ? w - 1 : 0, (c & 1) ? w - 1 : 0, my_start, my_n);
    int st[4], ln[4], cum[5];
    cum[0] = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        st[k] = __builtin_amdgcn_readlane(my_start, k);
        ln[k] = (k >= ph0 && k < ph1) ? __builtin_amdgcn_readlane(my_n, k) : 0;
        cum[k + 1] = cum[k] + ((ln[k] + 63) >> 6);           // instructions of taps 0..k
    }
    const int ninstr = cum[4];
    const unsigned acc_addr = (unsigned)(size_t)(air_lds_float*)(sh_acc + c);
    for (int base = 0; base < ninstr; base += 128) {
        // the instruction list is tabulated in registers, lane l holding entries base + l and
        // base + 64 + l (first-term offset, valid lanes); the issue loop below reads them with
        // v_readlane and stays a few hundred instructions long (a fully unrolled state machine
        // over taps x chunks grew to tens of thousands and ran out of the instruction cache)
        int ent_a[2], ent_n[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int i = base + h * 64 + lane;
            const int ph = (i >= cum[1]) + (i >= cum[2]) + (i >= cum[3]);
            const int k0 = (i - (ph == 0 ? cum[0] : ph == 1 ? cum[1] : ph == 2 ? cum[2] : cum[3])) * 64;
            ent_a[h] = (ph == 0 ? st[0] : ph == 1 ? st[1] : ph == 2 ? st[2] : st[3]) + k0;
            ent_n[h] = i < ninstr ? min(64, (ph == 0 ? ln[0] : ph == 1 ? ln[1] : ph == 2 ? ln[2] : ln[3]) - k0) : 0;
        }
        const int m = min(128, ninstr - base);
        // One batch: 16 reads in two asm statements of 8, each statement ENDING with its own s_waitcnt -- when the
        // statement is over its outputs are architecturally valid, so the compiler may move, copy or spill them freely
        // (it cannot see LDS returns in flight across asm statements).  The reads queue behind the previous
        // batch's adds (a wave's LDS operations execute in order), i.e. the wait also drains those: the atomic pipe
        // idles only for the ~2 x 100 cycles of the two read round trips per 16 x 255-cycle batch.
        auto batch = [&](int j0) {
            float r[NB];
            int d[NB];
            unsigned ad[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int j = j0 + u;                          // uniform
                d[u] = 0; ad[u] = (unsigned)(size_t)(air_lds_float*)sh_T;
                if (j < m) {
                    const int a0 = __builtin_amdgcn_readlane(j < 64 ? ent_a[0] : ent_a[1], j & 63);
                    d[u] = __builtin_amdgcn_readlane(j < 64 ? ent_n[0] : ent_n[1], j & 63);
                    ad[u] = (unsigned)(size_t)(air_lds_float*)(sh_T + a0 + min(lane, max(d[u] - 1, 0)));
                }
            }
#pragma unroll
            for (int h = 0; h < NB; h += 8)
                asm volatile("ds_read_b32 %0, %8\n ds_read_b32 %1, %9\n ds_read_b32 %2, %10\n ds_read_b32 %3, %11\n"
                             "ds_read_b32 %4, %12\n ds_read_b32 %5, %13\n ds_read_b32 %6, %14\n ds_read_b32 %7, %15\n"
                             "s_waitcnt lgkmcnt(0)"
                             : "=&v"(r[h]), "=&v"(r[h + 1]), "=&v"(r[h + 2]), "=&v"(r[h + 3]),
                               "=&v"(r[h + 4]), "=&v"(r[h + 5]), "=&v"(r[h + 6]), "=&v"(r[h + 7])
                             : "v"(ad[h]), "v"(ad[h + 1]), "v"(ad[h + 2]), "v"(ad[h + 3]),
                               "v"(ad[h + 4]), "v"(ad[h + 5]), "v"(ad[h + 6]), "v"(ad[h + 7])
                             : "memory");
#pragma unroll
            for (int u = 0; u < NB; ++u)
                if (lane < d[u]) asm volatile("ds_add_f32 %0, %1" :: "v"(acc_addr), "v"(r[u]) : "memory");   // valid lanes only (EXEC)
        };
#pragma unroll 1
        for (int j0 = 0; j0 < m; j0 += NB) batch(j0);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// The SECOND sequential accumulator: a ring over the lanes of one wave.  Lane k holds term k of a batch of 64 (one
// coalesced ds_read_b32), the running sum travels S[k] = S[k-1] + r[k] with one v_add_f32 ... wave_ror:1 per term, lane
// 63 carries it into the next batch (lane 0 reads lane 63); padding lanes hold -0.0f (x + -0 == x).  12 cycles per
// term against the pipe's 4 and a register chain's 8.4 -- but it needs ONE LDS request per 64 terms and no per-lane
// control flow, and the four corners run on the four SIMDs at once: tools/exp/dpp_chain.hip.
// A DPP operand reading the previous instruction's result formally wants two wait states; gfx950 interlocks it
// (bit-exact over 10^4-term streams without them, 16.4 cycles with s_nop 0, 18.2 with s_nop 1) -- probed at load time
// like the pipe's lane order (accumulators()).
template <bool ALLPH>
__device__ __forceinline__ void ring_corner(const WbCtx& ctx, int c, int ph0, int ph1) {
    const int lane = ctx.lane, w = ctx.w;
    float* const sh_T = ctx.sh_T;
    float* const sh_acc = ctx.sh_acc;
    float S = sh_acc[c];                                  // (lane 63's copy is the accumulator)
    // a ring issues one dependent instruction every 12 cycles and idles in between: at the top issue priority it keeps
    // that cadence beside the other waves of its SIMD (the pixel loop, the other workgroup's term phase)
    __builtin_amdgcn_s_setprio(3);
    for (int ph = ph0; ph < ph1; ++ph) {
        int start, n;
        slot_run<ALLPH>(ctx, ph, (c & 2) ? w - 1 : 0, (c & 1) ? w - 1 : 0, start, n);
        start = __builtin_amdgcn_readfirstlane(start); n = __builtin_amdgcn_readfirstlane(n);
        if (n <= 0) continue;
        // RD batches of 64 terms are read ahead of the adds: beside a feeding wave the LDS serves a read only after the
        // atomics queued in front of it (up to 16 instructions of ~255 cycles per feeding wave), i.e. thousands of cycles
        // late -- with ONE batch in flight (768 cycles of adds) a ring beside the pipe ran at a fraction of its 12
        // cycles per term
        constexpr int RD = 8;
        float r[RD];
#pragma unroll
        for (int d = 0; d < RD; ++d) { const int ix = d * 64 + lane; r[d] = ix < n ? sh_T[start + ix] : -0.0f; }
        for (int b = 0; b < n; b += 64 * RD) {
#pragma unroll
            for (int d = 0; d < RD; ++d) {
                if (b + d * 64 < n) {                                   // (uniform)
#pragma unroll
                    for (int k = 0; k < 64; ++k)
                        asm volatile("v_add_f32_dpp %0, %0, %1 wave_ror:1 row_mask:0xf bank_mask:0xf" : "+v"(S) : "v"(r[d]));
                }
                const int nx = b + (d + RD) * 64 + lane;
                r[d] = nx < n ? sh_T[start + nx] : -0.0f;               // refill this slot: RD batches ahead
            }
        }
    }
    __builtin_amdgcn_s_setprio(0);
    if (lane == 63) sh_acc[c] = S;
}
// corner c's streams of taps ph0 .. ph1-1 on the accumulator this part has: the LDS atomic pipe, or -- the pipe does not
// order lanes -- the lane ring.  (A per-workgroup MIX / split -- the k largest corners on the pipe, the others as rings
// beside it, k minimising max(4 x pipe terms, 12 x longest ring) -- was built and measured in rounds 3 / 4: bit-identical,
// and no faster at either configuration (0.1806 / 0.716 ms with the pipe alone, 0.1807 / 0.715-0.726 split): the pipe runs
// at its uncontended 4.0 cycles per term even with two workgroups per CU, and the launch waits for the workgroup whose ONE
// corner owns everything.  DESIGN.md sections 8 and 9.  Removed.  The rings are the fallback of a part whose pipe is not
// ordered: 0.195 / 0.840 ms, against 0.207 / 1.214 ms for the register chains.)
template <bool ALLPH>
__device__ __forceinline__ void corner_accumulate(const WbCtx& k, int c, int ph0, int ph1, bool lds_ordered, bool ring_ok) {
    if (lds_ordered) feed_corner<ALLPH>(k, c, ph0, ph1);
    else if (ring_ok) ring_corner<ALLPH>(k, c, ph0, ph1);
}

// ---- the pixel loop: theta / z gradients, per canvas pixel -------------------------------------------------------------
// The NT threads tid0 .. tid0 + NT - 1 share the canvas, three pixels in flight per thread.  NO LDS access: the loop runs on
// waves 4..15 WHILE waves 0..3 push the corner terms through the LDS atomic pipe (whose traffic starves every other LDS
// request of the CU), so the taps are recomputed per pixel (axis_tap: the same function of the same inputs as the tables)
// and d_recon / the window come from memory (L1 / L2: 10 KB + 3 KB per workgroup at 50 x 50).
// FOLD: d_recon of this image exists in sh_g only (its owner's stores are for the launches behind this one), so the
// values of this thread's pixels -- pixel m of the loop below is tt + m * NT -- are taken into registers while the LDS
// still answers at full speed (theta_take, before the corner feeds start): THETA_G per thread cover the canvas
constexpr int THETA_G = 6;
__device__ __forceinline__ void theta_take(const WbCtx& k, int tid0, int NT, float (&theta_g)[THETA_G]) {
#pragma unroll
    for (int m = 0; m < THETA_G; ++m) { const int p = k.tid - tid0 + m * NT; theta_g[m] = (p >= 0 && p < k.CC) ? k.sh_g[p] : 0.0f; }
}
// one round of the loop: pixels p0, p0 + NT, p0 + 2 NT (FOLD: round IT of theta_g)
template <bool FOLD, int IT>
__device__ __forceinline__ void theta_round(const WbCtx& k, int p0, int NT, const float (&theta_g)[THETA_G], WbGrad& G) {
    const int C = k.C, w = k.w, CC = k.CC;
    const float* v = k.v;
    Tap tx[3], ty[3];
    float Iv[3][4], gv[3], tj[3], ti[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int p = min(p0 + q * NT, CC - 1), i = p / C, j = p - i * C;
        if constexpr (FOLD) gv[q] = theta_g[IT * 3 + q];
        else gv[q] = (p0 + q * NT < CC) ? k.gsrc[p] : 0.0f;     // a pixel past the end contributes exact zeros
        tx[q] = axis_tap(j, C, w, k.ia, k.bx, &tj[q]); ty[q] = axis_tap(i, C, w, k.ia, k.by, &ti[q]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        Iv[q][0] = v[ty[q].i0 * w + tx[q].i0]; Iv[q][1] = v[ty[q].i1 * w + tx[q].i0];
        Iv[q][2] = v[ty[q].i0 * w + tx[q].i1]; Iv[q][3] = v[ty[q].i1 * w + tx[q].i1];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        G.dz += gv[q] * bilinear4(tx[q], ty[q], Iv[q][0], Iv[q][1], Iv[q][2], Iv[q][3]);   // canvas/mul_grad: Select_grad * window_recon
        float gX, gY;
        graph_dxy(k.z * gv[q], Iv[q][0], Iv[q][1], Iv[q][2], Iv[q][3], tx[q], ty[q], (float)w - 1.001f, gX, gY);
        G.d00 += gX * tj[q]; G.d02 += gX;                    // MatMul_grad: rows of theta x (x_t, y_t, 1)
        G.d11 += gY * ti[q]; G.d12 += gY;
    }
}
template <bool FOLD>
__device__ __forceinline__ void theta_loop(const WbCtx& k, int tid0, int NT, const float (&theta_g)[THETA_G], WbGrad& G) {
    const int tt = k.tid - tid0;
    if (tt < 0 || tt >= NT) return;
    if constexpr (FOLD) {
        static_assert(THETA_G == 6, "two rounds of three pixels");
        if (tt < k.CC) theta_round<true, 0>(k, tt, NT, theta_g, G);
        if (tt + 3 * NT < k.CC) theta_round<true, 1>(k, tt + 3 * NT, NT, theta_g, G);
    } else {
        for (int p0 = tt; p0 < k.CC; p0 += 3 * NT) theta_round<false, 0>(k, p0, NT, theta_g, G);
    }
    publish_wave_partials(k, G);
}
// theta_recon = [[1/s, 0, -x/s], [0, 1/s, -y/s]] (air_model.py:353-356): truediv_grad .. truediv_3_grad,
// summed in AddN_24's order; Neg_grad / Neg_1_grad for x, y.  One wave: lanes 0..4 each combine one quantity over
// the waves' partials in wave order; lane 0 collects them by shuffle
__device__ __forceinline__ void finish_theta(const WbCtx& k) {
    const float s = k.s, x = k.x, y = k.y;
    float u = 0.0f;
    if (k.lane < 5) { u = k.sh_red[k.lane]; for (int wv = 1; wv < WB_NW; ++wv) u += k.sh_red[wv * 8 + k.lane]; }
    float t5[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) t5[q] = __shfl(u, q, 64);
    if (k.lane == 0) {
        const float n1 = (-1.0f / s) / s;
        k.dsx[0] = ((t5[0] * n1 + t5[1] * ((x / s) / s)) + t5[2] * n1) + t5[3] * ((y / s) / s);
        k.dsx[1] = -(t5[1] / s);
        k.dsx[2] = -(t5[3] / s);
        k.dsx[3] = t5[4];
    }
}
// the tail of the graph-order bodies, behind the last corner feed's barrier: the corner slots' outputs from their
// accumulators, the theta / z outputs
__device__ __forceinline__ void graph_tail(const WbCtx& k, const WbSlot& s) {
    AIR_STAMP(45);
    if (s.corner) wb_store_slot(k, k.tid, k.sh_acc[(s.sp ? 2 : 0) + (s.sq ? 1 : 0)]);
    if (k.tid < 64) finish_theta(k);
}

// ---- corners and slots, carried order --------------------------------------------------------------------------------------
// The chunk walk over a group of lanes first .. first + count - 1 that hold one chunk each, in stream order.  ck = the
// chunk's sum from +0.0: P (pk) = the exclusive running sum of the ck's, continued from `run` ...
__device__ __forceinline__ void chunk_prefix(float ck, int lane, int first, int count, float& run, float& pk) {
#pragma unroll
    for (int l = first; l < first + count; ++l) {
        pk = lane == l ? run : pk;
        run += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ck), l));
    }
}
// ... and, qk = the chunk's chain from its P: the corrections Q_k - P_k+1 of the chunks before the last, added in stream
// order (empty chunks: nothing); qprev ends as Q_last.  corr / qprev / have continue from tap to tap
__device__ __forceinline__ void chunk_corrections(int len, float pk, float qk, int first, int count, float& corr, float& qprev, bool& have) {
#pragma unroll
    for (int l = first; l < first + count; ++l) {
        if (__builtin_amdgcn_readlane(len, l) > 0) {             // (uniform)
            if (have) corr += qprev - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pk), l));
            qprev = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qk), l));
            have = true;
        }
    }
}
// all taps resident: corner `c` on one wave, lane = tap * 16 + chunk.  [C of every chunk] -> [P: their exclusive running sum
// in stream order] -> [Q of every chunk from its P] -> [the running sum of Q - P in stream order]
__device__ __forceinline__ void carried_corner_wave(const WbCtx& k, int c) {
    const int lane = k.lane;
    int cp, cq, start, n;
    corner_pq(c, k.w, cp, cq);
    slot_run<true>(k, lane >> 4, cp, cq, start, n);
    n = max(n, 0);
    int nmax = n;
#pragma unroll
    for (int m = 16; m < 64; m <<= 1) nmax = max(nmax, __shfl_xor(nmax, m, 64));
    if (nmax <= WB_CHUNK_MIN) {
        // all four streams are single chunks: the reference's chain (lanes 0, 16, 32, 48 hold the taps' runs)
        float du = 0.0f;
#pragma unroll
        for (int ph = 0; ph < 4; ++ph)
            du = stream_add(du, k.sh_T, __builtin_amdgcn_readlane(start, ph * 16), __builtin_amdgcn_readlane(n, ph * 16));
        if (lane == 0) publish_corner(k, c, du);
    } else {
        const int cs = wb_chunk_len(n), off = (lane & 15) * cs, len = min(max(n - off, 0), cs);
        const float ck = stream_add(0.0f, k.sh_T, start + off, len);
        float run = 0.0f, pk = 0.0f;
        chunk_prefix(ck, lane, 0, 64, run, pk);
        const float qk = stream_add(pk, k.sh_T, start + off, len);
        float corr = 0.0f, qprev = 0.0f;
        bool have = false;
        chunk_corrections(len, pk, qk, 0, 64, corr, qprev, have);
        if (lane == 0) publish_corner(k, c, qprev + corr);
    }
}
// one tap per pass: ONE wave holds the four corners' chunks of the pass (lane = corner * 16 + chunk) and carries the corner
// accumulators from pass to pass.  P = the four corners' prefixes, Q / corr / have = the last chain's end, the
// corrections so far and whether a chain has run (acc = Q + corr; a short corner -- all four streams single chunks -- keeps
// the reference's chain in acc)
__device__ __forceinline__ void carried_corners_open(const WbCtx& k, float (&cacc)[4], float (&cP)[4], float (&cQ)[4], float (&ccorr)[4], bool (&cshort)[4], bool (&chave)[4]) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) {
            int p, q, st, n;
            corner_pq(c, k.w, p, q);
            slot_run<false>(k, ph, p, q, st, n);
            cshort[c] = cshort[c] && n <= WB_CHUNK_MIN;
        }
}
template <int PH>
__device__ __forceinline__ void carried_corners_pass(const WbCtx& k, float (&cacc)[4], float (&cP)[4], float (&cQ)[4], float (&ccorr)[4], bool (&cshort)[4], bool (&chave)[4]) {
    // lane = corner * 16 + chunk of this pass's tap
    const int lane = k.lane;
    int p, q, start, n;
    corner_pq(lane >> 4, k.w, p, q);
    slot_run<false>(k, PH, p, q, start, n);
    n = max(n, 0);
    const int cs = wb_chunk_len(n), off = (lane & 15) * cs, len = min(max(n - off, 0), cs);
    const float ck = stream_add(0.0f, k.sh_T, start + off, len);
    float pk = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float run = cshort[c] ? cacc[c] : cP[c];          // (a short corner continues the reference's chain)
        chunk_prefix(ck, lane, c * 16, 16, run, pk);
        cP[c] = run;
    }
    const float qk = stream_add(pk, k.sh_T, start + off, len);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (cshort[c]) { cacc[c] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, qk), c * 16)); continue; }
        chunk_corrections(len, pk, qk, c * 16, 16, ccorr[c], cQ[c], chave[c]);
        cacc[c] = cQ[c] + ccorr[c];
    }
}
// a thread's own slot, taps [PH0, PH1).  short_s: all four of its streams are single chunks -> the reference's chain (acc);
// otherwise P_s / corr_s / Q_s carry the scheme from tap to tap (and from pass to pass on large canvases)
template <bool ALLPH>
__device__ __forceinline__ bool carried_slot_short(const WbCtx& k, const WbSlot& s) {
    bool short_s = true;
    if (s.is_slot) {
#pragma unroll
        for (int ph = 0; ph < 4; ++ph) { int st, n; slot_run<ALLPH>(k, ph, s.sp, s.sq, st, n); short_s = short_s && n <= WB_CHUNK_MIN; }
    }
    return short_s;
}
template <bool ALLPH, int PH0, int PH1>
__device__ __forceinline__ void carried_slot(const WbCtx& k, const WbSlot& s, float& P_s, float& corr_s, float& Q_s, bool short_s, bool& have_s,
                                             float& acc) {
    if (!s.is_slot) return;
#pragma unroll
    for (int ph = PH0; ph < PH1; ++ph) {
        int start, n;
        slot_run<ALLPH>(k, ph, s.sp, s.sq, start, n);
        n = max(n, 0);
        if (short_s) { acc = stream_add(acc, k.sh_T, start, n); continue; }
        const int cs = wb_chunk_len(n);
        for (int k0 = 0; k0 < n; k0 += cs) {
            if (have_s) corr_s += Q_s - P_s;                 // the previous chunk's chain against the prefix behind it (exact)
            float c = 0.0f, q = P_s;
            stream_add2(c, q, k.sh_T, start + k0, min(cs, n - k0));
            Q_s = q;
            P_s += c;
            have_s = true;
        }
        acc = Q_s + corr_s;                                  // (final after the last tap)
    }
}
// ---- the four bodies ----------------------------------------------------------------------------------------------------
// seq_flags (accumulators(), below): bit 0 the LDS atomic pipe applies lanes in order, bit 1 the lane-ring accumulator
// is exact on this part (used when the pipe is not)

// graph order, all four taps' terms resident (4*C*C floats of LDS, no barrier between taps):
// [terms of all taps] | [short chains + slot outputs on all waves: no LDS atomics in flight, every dependent LDS
// read returns at full speed] | [corner accumulation on the LDS || pixel loop on VALU / memory].
// While the atomic pipe runs, every other LDS request of the CU starves, so the short chains go first and the pixel
// loop -- which touches no LDS at all -- runs on the other twelve waves underneath it.
// FOLD: the compose front first (fold_front); an owner is counted beside the corner feeds and the means run behind the
// workgroup's own outputs
template <bool FOLD>
__device__ __forceinline__ void write_bwd_graph_allph_body(const air_write_bwd_t& a, int seq_flags, const air_write_fwd_t* fp,
                                                           int32_t* arrive) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const bool lds_ordered = seq_flags & 1, ring_ok = seq_flags & 2;
    WbCtx k = wb_ctx<true>(a, smem);
    const bool owner = FOLD && k.t == 0;
    float win_pre = 0.0f, g_pre[8];
    if constexpr (FOLD) {
        AIR_STAMP(40);
        AIR_STAMP_WG(0);
        if (!fold_front(a, *fp, arrive, k, owner, win_pre)) return;
    } else if (!wb_open<true>(a, k, win_pre, g_pre)) return;
    wb_setup<!FOLD>(k, win_pre, g_pre);
    const WbSlot s = wb_slot<false>(k, lds_ordered, ring_ok);
    WbGrad G = {0.f, 0.f, 0.f, 0.f, 0.f};
    float acc = 0.0f, theta_g[THETA_G];
    AIR_STAMP_WG(1);
    stage_terms<true, 0, 4>(k);
    __syncthreads();
    AIR_STAMP(43);
    AIR_STAMP_WG(2);
    chains<true>(k, s, 0, 4, acc);
    AIR_STAMP(49);
    publish(k, s, acc);
    if (FOLD) theta_take(k, WB_TH0, WB_THN, theta_g);
    AIR_STAMP(39);
    __syncthreads();
    AIR_STAMP(44);
    AIR_STAMP_WG(3);
    if (k.wave < 4) corner_accumulate<true>(k, k.wave, 0, 4, lds_ordered, ring_ok);
    else {
        // an owner is counted here, beside the corner feeds and long after its two words were stored: neither the wait
        // for those stores nor the add's round trip stands in front of a barrier
        const int ticket = owner ? fold_signal(arrive, k.tid) : -1;
        theta_loop<FOLD>(k, WB_TH0, WB_THN, theta_g, G);
        if (owner && k.tid == WB_SIG) *fold_last_word(k) = ticket == a.B - 1 ? 1 : 0;
    }
    AIR_STAMP(48);
    AIR_STAMP_WG(4);                       // wave 0's own feed is over
    __syncthreads();
    AIR_STAMP_WG(5);
    graph_tail(k, s);
    if (owner) fold_means(a, arrive, k, *fold_last_word(k) != 0);      // (behind this workgroup's own outputs: nothing waits for the means)
    AIR_STAMP(47);
    AIR_STAMP_WG(6);
}

// graph order, one tap at a time through one buffer (large canvases): per tap [terms] | [chains] | [corner feed || pixel loop
// in pass 0]
__device__ __forceinline__ void write_bwd_graph_onetap_body(const air_write_bwd_t& a, int seq_flags) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const bool lds_ordered = seq_flags & 1, ring_ok = seq_flags & 2;
    WbCtx k = wb_ctx<false>(a, smem);
    float win_pre = 0.0f, g_pre[8];
    if (!wb_open<false>(a, k, win_pre, g_pre)) return;
    wb_setup<false>(k, win_pre, g_pre);
    const WbSlot s = wb_slot<false>(k, lds_ordered, ring_ok);
    WbGrad G = {0.f, 0.f, 0.f, 0.f, 0.f};
    float acc = 0.0f, theta_g[THETA_G];
    // (debug stamps of every workgroup: [1] terms, [2] chains, [3] corner phase summed over the four passes, [4] hardware
    // id (XCC / SE / CU), [5] pipe mask, [6] end; tools/wb_wg_stamps.py --stress)
    AIR_STAMP_WG_SET(1, 0); AIR_STAMP_WG_SET(2, 0); AIR_STAMP_WG_SET(3, 0);
    AIR_STAMP_WG_SET(4, (__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) << 16) | __builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)));
    AIR_STAMP_WG_SET(5, (lds_ordered ? 0xf : 0) | (k.sh_cn[0] + k.sh_cn[1] + k.sh_cn[2] + k.sh_cn[3]) << 4);
    for (int ph = 0; ph < 4; ++ph) {
        const unsigned long long ta = AIR_NOW();
        if (ph == 0) stage_terms<false, 0, 1>(k);
        else if (ph == 1) stage_terms<false, 1, 2>(k);
        else if (ph == 2) stage_terms<false, 2, 3>(k);
        else stage_terms<false, 3, 4>(k);
        __syncthreads();
        AIR_STAMP(50 + 3 * ph);
        AIR_STAMP_WG_ADD(1, ta);
        const unsigned long long tb = AIR_NOW();
        chains<false>(k, s, ph, ph + 1, acc);
        __syncthreads();
        AIR_STAMP(51 + 3 * ph);
        AIR_STAMP_WG_ADD(2, tb);
        const unsigned long long tc = AIR_NOW();
        if (k.wave < 4) corner_accumulate<false>(k, k.wave, ph, ph + 1, lds_ordered, ring_ok);
        else if (ph == 0) theta_loop<false>(k, WB_TH0, WB_THN, theta_g, G);
        __syncthreads();
        AIR_STAMP(52 + 3 * ph);
        AIR_STAMP_WG_ADD(3, tc);
    }
    publish(k, s, acc);
    __syncthreads();
    graph_tail(k, s);
    AIR_STAMP(47);
    AIR_STAMP_WG(6);
}

// carried order, all taps resident:
// [terms of all taps + coordinate gradients] | [waves 0..3: corner c's 4 x 16 chunks, one per lane, then their 64
// sums added in stream order || the other slots' streams, one lane each || last wave: the theta / z outputs]
__device__ __forceinline__ void write_bwd_carried_allph_body(const air_write_bwd_t& a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    WbCtx k = wb_ctx<true>(a, smem);
    float win_pre = 0.0f, g_pre[8];
    if (!wb_open<true>(a, k, win_pre, g_pre)) return;
    wb_setup<true>(k, win_pre, g_pre);
    const WbSlot s = wb_slot<true>(k, false, false);
    WbGrad G = {0.f, 0.f, 0.f, 0.f, 0.f};
    float acc = 0.0f;
    float P_s = 0.0f, corr_s = 0.0f, Q_s = 0.0f;
    bool have_s = false;
    const bool short_s = carried_slot_short<true>(k, s);
    AIR_STAMP_WG(1);
    carried_terms<true, 0, 4, true>(k, G);
    publish_wave_partials(k, G);
    __syncthreads();
    AIR_STAMP(43);
    AIR_STAMP_WG(2);
    if (k.wave < 4) carried_corner_wave(k, k.wave);
    if (k.wave == WB_NW - 1) finish_theta(k);
    AIR_STAMP(44);
    AIR_STAMP_WG(3);
    carried_slot<true, 0, 4>(k, s, P_s, corr_s, Q_s, short_s, have_s, acc);
    AIR_STAMP_WG(4);
    AIR_STAMP_WG_T(5, 4 * 64);
    publish(k, s, acc);
    AIR_STAMP(47);
    AIR_STAMP_WG(6);
    AIR_STAMP_WG_T(7, 15 * 64);
}

// carried order, one tap per pass (large canvases).  Wave 1 holds the four corners' chunks of the pass and carries the
// corner accumulators from pass to pass; the coordinate gradients ride in pass 0
__device__ __forceinline__ void write_bwd_carried_onetap_body(const air_write_bwd_t& a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    WbCtx k = wb_ctx<false>(a, smem);
    float win_pre = 0.0f, g_pre[8];
    if (!wb_open<false>(a, k, win_pre, g_pre)) return;
    wb_setup<false>(k, win_pre, g_pre);
    const WbSlot s = wb_slot<true>(k, false, false);
    WbGrad G = {0.f, 0.f, 0.f, 0.f, 0.f};
    float acc = 0.0f;
    float P_s = 0.0f, corr_s = 0.0f, Q_s = 0.0f;
    bool have_s = false;
    const bool short_s = carried_slot_short<false>(k, s);
    float cacc[4] = {0.f, 0.f, 0.f, 0.f}, cP[4] = {0.f, 0.f, 0.f, 0.f}, cQ[4] = {0.f, 0.f, 0.f, 0.f}, ccorr[4] = {0.f, 0.f, 0.f, 0.f};
    bool cshort[4] = {true, true, true, true}, chave[4] = {false, false, false, false};
    if (k.wave == 1) carried_corners_open(k, cacc, cP, cQ, ccorr, cshort, chave);
    // one pass: tap PH's terms (the coordinate gradients ride in pass 0), the corners' chunks on wave 1, every other slot's
    // stream.  (A local lambda, not a part: as a free function, or written out four times, the kernel takes 74 VGPRs instead
    // of 70 and loses a wave per SIMD -- DESIGN.md section 32)
    auto pass = [&](auto phc) __attribute__((always_inline)) {
        constexpr int PH = decltype(phc)::value;
        carried_terms<false, PH, PH + 1, PH == 0>(k, G);
        if (PH == 0) publish_wave_partials(k, G);
        __syncthreads();
        if (k.wave == 1) carried_corners_pass<PH>(k, cacc, cP, cQ, ccorr, cshort, chave);
        if (PH == 0 && k.wave == WB_NW - 1) finish_theta(k);
        carried_slot<false, PH, PH + 1>(k, s, P_s, corr_s, Q_s, short_s, have_s, acc);
        if (PH < 3) __syncthreads();
    };
    pass(std::integral_constant<int, 0>{}); pass(std::integral_constant<int, 1>{});
    pass(std::integral_constant<int, 2>{}); pass(std::integral_constant<int, 3>{});
    publish(k, s, acc);
    if (k.wave == 1 && k.lane < 4)
        publish_corner(k, k.lane, k.lane == 0 ? cacc[0] : k.lane == 1 ? cacc[1] : k.lane == 2 ? cacc[2] : cacc[3]);
    AIR_STAMP(47);
    AIR_STAMP_WG(6);
}

template <bool ALLPH>
__global__ __launch_bounds__(WB_THREADS) void write_bwd_graph_kernel(air_write_bwd_t a, int seq_flags)
{
    if constexpr (ALLPH) write_bwd_graph_allph_body<false>(a, seq_flags, nullptr, nullptr);
    else write_bwd_graph_onetap_body(a, seq_flags);
}
template <bool ALLPH>
__global__ __launch_bounds__(WB_THREADS) void write_bwd_carried_kernel(air_write_bwd_t a)
{
    if constexpr (ALLPH) write_bwd_carried_allph_body(a);
    else write_bwd_carried_onetap_body(a);
}
// compose + the graph-order write backward in one launch (air_write_fwd_bwd)
__global__ __launch_bounds__(WB_THREADS) void compose_write_bwd_graph_kernel(air_write_fwd_t f, air_write_bwd_t a, int32_t* arrive, int seq_flags)
{
    write_bwd_graph_allph_body<true>(a, seq_flags, &f, arrive);
}

// ---------------------------------------------------------------------------
// The bit-for-bit reproduction of the reference's UnsortedSegmentSum rests on a property of gfx950 that no manual
// states: a same-address ds_add_f32 applies the 64 lanes of an instruction in ascending lane order, and a wave's
// instructions in program order.  It is probed ONCE per process and device on the first eager call that needs it (a
// known-order sum whose value depends on the order; the probe needs a stream synchronise, so a first call under stream
// capture takes the register chains -- nothing is assumed -- and says so: capture_graph() warms up eagerly first).  A
// part that orders differently takes the ring / register-chain fallbacks (same results, slower) instead of silently
// changing gradients.
// AIR_LDS_ORDER=0 / 1 forces the answer (tests run both paths against each other).
// ---------------------------------------------------------------------------
constexpr int PROBE_N = 8 * 64;
__device__ float air_probe_vals[PROBE_N];
__device__ float air_probe_out[4];
__global__ void lds_order_probe_kernel() {
    __shared__ float slot[2];
    if (threadIdx.x < 2) slot[threadIdx.x] = 0.0f;
    __syncthreads();
    for (int k = 0; k < PROBE_N / 64; ++k) lds_fadd(&slot[0], air_probe_vals[k * 64 + threadIdx.x]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) air_probe_out[0] = slot[0];
    // the lane ring of write_bwd_graph_kernel (ring_corner) on the same stream: the same value if the DPP read of the
    // previous instruction's result is interlocked and wave_ror:1 hands lane k-1 (63 for lane 0) to lane k
    float S = 0.0f;
    for (int k = 0; k < PROBE_N / 64; ++k) {
        const float r = air_probe_vals[k * 64 + threadIdx.x];
#pragma unroll
        for (int i = 0; i < 64; ++i)
            asm volatile("v_add_f32_dpp %0, %0, %1 wave_ror:1 row_mask:0xf bank_mask:0xf" : "+v"(S) : "v"(r));
    }
    if (threadIdx.x == 63) air_probe_out[1] = S;
}

// bit 0: the LDS atomic pipe is a sequential accumulator on this part; bit 1: so is the lane ring.
// Remembered PER DEVICE (a node may mix parts).  A first call that arrives while the stream is being captured cannot
// probe (the probe synchronises): it takes the conservative answer -- neither property, i.e. the register chains, same
// bits on any part, slower -- says so once, and remembers nothing, so the first eager call still probes.
int accumulators(hipStream_t s) {
    constexpr int MAX_DEV = 32;
    static std::atomic<int> states[MAX_DEV];             // per device: 0 unknown, else 4 | flags
    static std::atomic<int> warned{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) dev = 0;
    std::atomic<int>& state = states[dev];
    int st = state.load(std::memory_order_acquire);
    if (st) return st & 3;
    const char* e0 = getenv("AIR_LDS_ORDER");
    const char* e1 = getenv("AIR_WB_RING");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
    int probed = 3;
    if (!(e0 && e1)) {
        if (capturing) {                                 // cannot synchronise here: nothing assumed, nothing remembered
            if (!warned.exchange(1))
                fprintf(stderr, "libair_hip: air_write_bwd / air_transformer_bwd first called under stream capture on device %d: the "
                                "accumulator probe cannot run, this capture takes the register-chain fallback (same results, slower) -- "
                                "run the launch once eagerly before capturing\n", dev);
            return (e0 ? (e0[0] != '0') : 0) | (e1 ? (e1[0] != '0') << 1 : 0);
        }
        float vals[PROBE_N];
        unsigned x = 12345u;
        float want = 0.0f;
        for (int i = 0; i < PROBE_N; ++i) {
            x = x * 1664525u + 1013904223u;
            // magnitudes over 2^-8 .. 2^23 with mixed signs: every partial sum rounds, so the value pins the order
            const float mant = 1.0f + (float)((x >> 9) & 0x3fffu) / 16384.0f;
            const int ex = (int)((x >> 24) & 31u) - 8;
            vals[i] = ((x >> 31) ? -1.0f : 1.0f) * ldexpf(mant, ex);
            want = want + vals[i];                           // ascending lane, program order
        }
        float got[2] = {0.0f, 0.0f};
        bool ok = hipMemcpyToSymbolAsync(HIP_SYMBOL(air_probe_vals), vals, sizeof(vals), 0, hipMemcpyHostToDevice, s) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(lds_order_probe_kernel, dim3(1), dim3(64), 0, s);
            ok = hipGetLastError() == hipSuccess &&
                 hipMemcpyFromSymbolAsync(got, HIP_SYMBOL(air_probe_out), sizeof(got), 0, hipMemcpyDeviceToHost, s) == hipSuccess &&
                 hipStreamSynchronize(s) == hipSuccess;
        }
        probed = ((ok && memcmp(&got[0], &want, sizeof(float)) == 0) ? 1 : 0) | ((ok && memcmp(&got[1], &want, sizeof(float)) == 0) ? 2 : 0);
        if (!(probed & 1) && !e0)
            fprintf(stderr, "libair_hip: ds_add_f32 lane order differs on this part (probe %.9g, expected %.9g): "
                            "the sampler backward takes its ring / register-chain fallbacks\n", (double)got[0], (double)want);
        if (!(probed & 2) && !e1)
            fprintf(stderr, "libair_hip: the DPP lane ring is not an in-order accumulator on this part (probe %.9g, expected %.9g): "
                            "the sampler backward keeps every corner stream on the LDS atomic pipe\n", (double)got[1], (double)want);
    }
    int flags = probed;
    if (e0) flags = (flags & 2) | (e0[0] != '0' ? 1 : 0);
    if (e1) flags = (flags & 1) | (e1[0] != '0' ? 2 : 0);
    state.store(4 | flags, std::memory_order_release);
    return flags;
}
int lds_ordered(hipStream_t s) { return accumulators(s) & 1; }

}  // namespace

extern "C" int air_transformer_bwd(const float* U, const float* theta, const float* d_out, float* d_U, float* d_theta,
                                   int B, int Hi, int Wi, int Ho, int Wo, void* stream) {
    if (!U || !theta || !d_out || (!d_U && !d_theta) || B <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return AIR_EINVAL;
    const size_t lds = (40 + 2 * (((size_t)Hi * Wi + 3) & ~3)) * sizeof(float);
    int rc = ensure_lds(transformer_bwd_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(transformer_bwd_kernel, dim3(B), dim3(THREADS), lds, air_stream(stream),
                       U, theta, d_out, d_U, d_theta, Hi, Wi, Ho, Wo, d_U ? lds_ordered(air_stream(stream)) : 1);
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int air_transformer_nc_bwd(const float* U, const float* theta, const float* d_out, float* d_U, float* d_theta,
                                      int B, int T, int Hi, int Wi, int C, int Ho, int Wo, void* stream) {
    if (!U || !theta || !d_out || (!d_U && !d_theta) || B <= 0 || T <= 0 || Hi <= 0 || Wi <= 0 || C <= 0 || Ho <= 0 || Wo <= 0)
        return AIR_EINVAL;
    // the bound of air_transformer_bwd on one channel's planes
    const size_t NIp = ((size_t)Hi * Wi + 3) & ~(size_t)3;
    if ((40 + 2 * NIp) * sizeof(float) > AIR_LDS_LIMIT) return AIR_ELIMIT;
    if ((long)Ho * Wo > INT32_MAX || (long)B * T > INT32_MAX) return AIR_ELIMIT;       // what the kernel indexes with an int
    // channels per d U workgroup: one per wave, as many as have their plane in LDS at once
    const size_t fit = (AIR_LDS_LIMIT / sizeof(float) - 32) / NIp;
    int cg = C < NC_WAVES ? C : NC_WAVES;
    if ((size_t)cg > fit) cg = (int)fit;                       // (fit >= 2 under the bound above)
    const int ngroups = d_U ? (C + cg - 1) / cg : 0;
    const long blocks = (long)B * ((long)ngroups + (d_theta ? T : 0));
    if (blocks > INT32_MAX) return AIR_ELIMIT;
    const size_t lds = (32 + (d_U ? (size_t)cg * NIp : 0)) * sizeof(float);
    int rc = ensure_lds(transformer_nc_bwd_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(transformer_nc_bwd_kernel, dim3((unsigned)blocks), dim3(THREADS), lds, air_stream(stream),
                       U, theta, d_out, d_U, d_theta, T, Hi, Wi, C, Ho, Wo, cg, ngroups, d_U ? lds_ordered(air_stream(stream)) : 1);
    AIR_CHECK_LAUNCH();
    return 0;
}

/* name of the kernel function air_write_bwd dispatches this descriptor to, as rocprofv3 prints it */
extern "C" int air_write_bwd_kernel_name(const air_write_bwd_t* a, char* buf, int n) {
    if (!a || !buf || n <= 0 || a->C < 2 || a->w < 2) return AIR_EINVAL;
    if (a->literal == 2 || a->literal == 4)
        snprintf(buf, n, "write_bwd_%s_kernel<%s>", a->literal == 4 ? "carried" : "graph",
                 write_bwd_graph_allph(a->C, a->w) ? "true" : "false");
    else snprintf(buf, n, "write_bwd_kernel");
    return 0;
}

extern "C" int air_write_bwd(const air_write_bwd_t* a, void* stream) {
    if (!a || !a->d_recon || !a->vrec || !a->att || !a->d_gen_pre || !a->d_sxy_write) return AIR_EINVAL;
    if (a->B <= 0 || a->N <= 0 || a->C < 2 || a->w < 2) return AIR_EINVAL;
    if (a->literal != 0 && a->literal != 2 && a->literal != 4) return AIR_EINVAL;     // (1 and 3 were removed with ABI 5)
    if (a->order && a->literal < 2) return AIR_EINVAL;            // (the ordered form exists in the graph-order kernels only)
    if (2 * a->w > THREADS) return AIR_ELIMIT;
    if (a->literal == 4) {
        // the carried graph order: register chains only -- no LDS-atomic lane order to probe, capture-safe from the first call
        if (a->w * a->w > WB_THREADS) return AIR_ELIMIT;
        const bool allph = write_bwd_graph_allph(a->C, a->w);
        const size_t lds = write_bwd_graph_smem(a->C, a->w, allph);
        int rc = allph ? ensure_lds(write_bwd_carried_kernel<true>, lds) : ensure_lds(write_bwd_carried_kernel<false>, lds);
        if (rc) return rc;
        if (allph) hipLaunchKernelGGL(write_bwd_carried_kernel<true>, dim3(a->B, a->N), dim3(WB_THREADS), lds, air_stream(stream), *a);
        else hipLaunchKernelGGL(write_bwd_carried_kernel<false>, dim3(a->B, a->N), dim3(WB_THREADS), lds, air_stream(stream), *a);
        AIR_CHECK_LAUNCH();
        return 0;
    }
    if (a->literal == 2) {
        if (a->w * a->w > WB_THREADS) return AIR_ELIMIT;
        // all four taps' terms resident when they fit next to a second workgroup's share of the LDS
        const bool allph = write_bwd_graph_allph(a->C, a->w);
        const size_t lds = write_bwd_graph_smem(a->C, a->w, allph);
        int rc = allph ? ensure_lds(write_bwd_graph_kernel<true>, lds) : ensure_lds(write_bwd_graph_kernel<false>, lds);
        if (rc) return rc;
        int flags = accumulators(air_stream(stream));
        if (allph) hipLaunchKernelGGL(write_bwd_graph_kernel<true>, dim3(a->B, a->N), dim3(WB_THREADS), lds, air_stream(stream), *a, flags);
        else hipLaunchKernelGGL(write_bwd_graph_kernel<false>, dim3(a->B, a->N), dim3(WB_THREADS), lds, air_stream(stream), *a, flags);
        AIR_CHECK_LAUNCH();
        return 0;
    }
    const size_t lds = write_bwd_smem(a->C, a->w);
    int rc = ensure_lds(write_bwd_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(write_bwd_kernel, dim3(a->B, a->N), dim3(WB_THREADS), lds, air_stream(stream), *a);
    AIR_CHECK_LAUNCH();
    return 0;
}

// ---------------------------------------------------------------------------
// air_write_fwd_bwd: air_write_fwd and air_write_bwd (literal 2, with the batch means) as ONE launch.  ONE host predicate
// says whether a descriptor pair has that form; the launcher and the name function both read it.
// ---------------------------------------------------------------------------
namespace {
int compose_fold_plan(const air_write_fwd_t* f, const air_write_bwd_t* b) {
    if (!f || !b) return AIR_EINVAL;
    if (!f->vrec || !f->ml || !f->images || !f->dyn || !f->att || !f->recon || !f->rec_loss || !f->d_recon ||
        !f->run_loss || !f->run_digits || !f->loss_item)
        return AIR_EINVAL;                                          // (d_recon: a train step)
    if (!b->d_gen_pre || !b->d_sxy_write || !b->fin_targets || !b->fin_scalars) return AIR_EINVAL;
    // the two descriptors describe one step: the backward reads what the forward leaves
    if (b->d_recon != f->d_recon || b->vrec != f->vrec || b->att != f->att || b->fin_loss_item != f->loss_item ||
        b->fin_digits != f->run_digits)
        return AIR_EINVAL;
    if (f->B <= 0 || f->N <= 0 || f->C < 2 || f->w < 2 || f->Z <= 0) return AIR_EINVAL;
    if (b->B != f->B || b->N != f->N || b->C != f->C || b->w != f->w) return AIR_EINVAL;
    if (b->literal != 2) return AIR_EINVAL;
    if (f->likelihood != AIR_LIK_BERNOULLI && f->likelihood != AIR_LIK_GAUSSIAN) return AIR_EINVAL;
    // the fold computes the Bernoulli likelihood only: any other keeps the two launches
    if (f->likelihood != AIR_LIK_BERNOULLI) return AIR_ELIMIT;
    if (f->N > MAX_STEPS || 2 * f->w > THREADS || f->w * f->w > WB_THREADS) return AIR_ELIMIT;
    // the hand-off of the batch means was measured with one workgroup per CU: no more items than the 256 CUs of the part
    // this is built for, hence no longest-first order either.  An assumption about placement, not a guarantee (two of
    // these workgroups fit a CU's LDS): include/air_hip.h says so
    if (f->wb_order || b->order || (long)f->N * f->B > 256) return AIR_ELIMIT;
    if (!write_bwd_graph_allph(f->C, f->w)) return AIR_ELIMIT;
    if (!compose_fold_fits(f->N, f->C, f->w)) return AIR_ELIMIT;
    if ((size_t)f->C * f->C > 6 * (size_t)(WB_THREADS - 4 * 64)) return AIR_ELIMIT;    // (THETA_G pixels per pixel-loop thread)
    return 0;
}
}  // namespace

extern "C" int air_write_fwd_bwd_kernel_name(const air_write_fwd_t* f, const air_write_bwd_t* b, char* buf, int n) {
    if (!buf || n <= 0) return AIR_EINVAL;
    const int rc = compose_fold_plan(f, b);
    if (rc) return rc;
    snprintf(buf, n, "compose_write_bwd_graph_kernel");
    return 0;
}

extern "C" int air_write_fwd_bwd(const air_write_fwd_t* f, const air_write_bwd_t* b, int32_t* arrive, void* stream) {
    int rc = compose_fold_plan(f, b);
    if (rc) return rc;
    if (!arrive) return AIR_EINVAL;
    const size_t lds = write_bwd_graph_smem(b->C, b->w, true);
    rc = ensure_lds(compose_write_bwd_graph_kernel, lds);
    if (rc) return rc;
    const int flags = accumulators(air_stream(stream));
    hipLaunchKernelGGL(compose_write_bwd_graph_kernel, dim3(b->B, b->N), dim3(WB_THREADS), lds, air_stream(stream), *f, *b, arrive, flags);
    AIR_CHECK_LAUNCH();
    return 0;
}
