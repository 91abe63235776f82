// Shared pieces of the sampler translation units (air_sampler.hip: the glimpse read, the heads around it, compose, the
// generic forward; air_sampler_write_bwd.hip: the write backward in its three orders, the generic backward, the lane-order
// probe; air_generate.hip: the records of generated scenes and the render-only compose): the per-axis tap of the
// axis-aligned transformer and the tap of the generic one, the reference's 4-product expression, the coordinate gradient
// in the saved graph's op order, the Concrete pre-sigmoid sample, and the staging / per-pixel code of compose.
#pragma once
#include "air_common.h"
#include <cstdio>
#include <atomic>
#include <type_traits>
#include <cstdlib>
#include <cstring>
#include <cmath>

namespace {

constexpr int THREADS = 256;

struct Tap { float w0, w1; int i0, i1; };   // w0 = (x1_f - x), w1 = (x - x0_f)

// transformer.py:75-87,108-115 for one output coordinate of one axis
__device__ __forceinline__ Tap axis_tap(int j, int n_out, int n_in, float a, float b, float* t_out = nullptr) {
    const float step = 2.0f / (float)(n_out - 1);
    const float t = (n_out > 1) ? (-1.0f + step * (float)j) : -1.0f;   // tf.linspace(-1, 1, n)
    const float xs = a * t + b;                                         // theta . (x_t, y_t, 1)
    const float X = ((xs + 1.0f) * ((float)n_in - 1.001f)) / 2.0f;
    const float f0 = floorf(X);
    const float lim = (float)(n_in - 1);
    const float c0 = fminf(fmaxf(f0, 0.0f), lim);          // clip AFTER floor / +1
    const float c1 = fminf(fmaxf(f0 + 1.0f, 0.0f), lim);
    Tap tp;
    tp.i0 = (int)c0; tp.i1 = (int)c1;
    tp.w0 = c1 - X;
    tp.w1 = X - c0;
    if (t_out) *t_out = t;
    return tp;
}

// literal transformer.py:108-116: wa*Ia + wb*Ib + wc*Ic + wd*Id, add_n left to right
__device__ __forceinline__ float bilinear4(const Tap& tx, const Tap& ty,
                                           float Ia, float Ib, float Ic, float Id) {
    const float wa = tx.w0 * ty.w0;
    const float wb = tx.w0 * ty.w1;
    const float wc = tx.w1 * ty.w0;
    const float wd = tx.w1 * ty.w1;
    return ((wa * Ia + wb * Ib) + wc * Ic) + wd * Id;
}

// one output pixel of the generic transformer (any theta), transformer.py:75-87,108-115,138-163: the meshgrid point, the
// source coordinates, the clipped corners and the per-axis weights taken from the CLIPPED corners
struct GenTap { float wx0, wx1, wy0, wy1; int x0, x1, y0, y1; float xt, yt; };
__device__ __forceinline__ GenTap generic_tap(const float* th, int i, int j, int Hi, int Wi, int Ho, int Wo) {
    GenTap t;
    t.xt = (Wo > 1) ? (-1.0f + (2.0f / (float)(Wo - 1)) * (float)j) : -1.0f;
    t.yt = (Ho > 1) ? (-1.0f + (2.0f / (float)(Ho - 1)) * (float)i) : -1.0f;
    const float xs = (th[0] * t.xt + th[1] * t.yt) + th[2] * 1.0f;
    const float ys = (th[3] * t.xt + th[4] * t.yt) + th[5] * 1.0f;
    const float X = ((xs + 1.0f) * ((float)Wi - 1.001f)) / 2.0f;
    const float Y = ((ys + 1.0f) * ((float)Hi - 1.001f)) / 2.0f;
    const float fx = floorf(X), fy = floorf(Y);
    const float x0 = fminf(fmaxf(fx, 0.f), (float)(Wi - 1)), x1 = fminf(fmaxf(fx + 1.f, 0.f), (float)(Wi - 1));
    const float y0 = fminf(fmaxf(fy, 0.f), (float)(Hi - 1)), y1 = fminf(fmaxf(fy + 1.f, 0.f), (float)(Hi - 1));
    t.wx0 = x1 - X; t.wx1 = X - x0; t.wy0 = y1 - Y; t.wy1 = Y - y0;
    t.x0 = (int)x0; t.x1 = (int)x1; t.y0 = (int)y0; t.y1 = (int)y1;
    return t;
}

// generic transformer backward, d theta: one output pixel's share.  ga..gd = g * Ia..Id (summed over the channels where
// there are several); graph_dxy's order (AddN over wa, wb, wc, wd) -- the two axes have their own (W - 1.001) here -- then the
// MatMul_grad contraction with (x_t, y_t, 1) into s6
__device__ __forceinline__ void generic_dtheta_pixel(const GenTap& t, float ga, float gb, float gc, float gd, int Hi, int Wi, float (&s6)[6]) {
    const float dX = ((-(ga * t.wy0) + -(gb * t.wy1)) + gc * t.wy0) + gd * t.wy1;
    const float dY = ((-(t.wx0 * ga) + t.wx0 * gb) + -(t.wx1 * gc)) + t.wx1 * gd;
    const float gX = (dX / 2.0f) * ((float)Wi - 1.001f);
    const float gY = (dY / 2.0f) * ((float)Hi - 1.001f);
    s6[0] += gX * t.xt; s6[1] += gX * t.yt; s6[2] += gX;
    s6[3] += gY * t.xt; s6[4] += gY * t.yt; s6[5] += gY;
}
// generic transformer backward, d U: weight (wa, wb, wc, wd) and input pixel of tap ph of one output pixel
__device__ __forceinline__ void generic_tap_term(const GenTap& t, int ph, int Wi, float& wgt, int& idx) {
    wgt = ((ph & 2) ? t.wx1 : t.wx0) * ((ph & 1) ? t.wy1 : t.wy0);
    idx = ((ph & 1) ? t.y1 : t.y0) * Wi + ((ph & 2) ? t.x1 : t.x0);
}

// Gradient of one output pixel wrt its source coordinates (X, Y) in the op order of the reference's SAVED graph
// (model/air-model.meta, executed by the graph executor of tests/test_graph_exec.py).  For an out-of-range pixel (both
// taps clipped to one index) the four legs cancel exactly in real arithmetic but NOT in fp32: the rounding residue,
// multiplied by g ~ 1 / (r + 1e-9) at unexplained ink, is not noise to be cleaned up -- it is the force that pulls glimpses
// towards unexplained ink, and the reference's training dynamics depend on it (with the exact adjoint the model does not
// learn to localise).  cx = (n_in - 1.001): x = (x_s + 1) * cx / 2.  d wa..wd = g*Ia..Id (mul_10..13_grad), each product's two factors get
// grad*other (mul_6..9_grad), the Sub nodes negate the (x1-x)/(y1-y) legs, and the four legs that
// reach x (y) are summed by AddN_10 / AddN_20 (AddN_11 / AddN_21) left to right in the order
// wa, wb, wc, wd.  Then x = (x_s + 1)*(W - 1.001)/2: truediv_grad then mul_grad.
__device__ __forceinline__ void graph_dxy(float g, float Ia, float Ib, float Ic, float Id,
                                          const Tap& tx, const Tap& ty, float cx, float& dxs, float& dys) {
    const float ga = g * Ia, gb = g * Ib, gc = g * Ic, gd = g * Id;
    const float dX = ((-(ga * ty.w0) + -(gb * ty.w1)) + gc * ty.w0) + gd * ty.w1;
    const float dY = ((-(tx.w0 * ga) + tx.w0 * gb) + -(tx.w1 * gc)) + tx.w1 * gd;
    dxs = (dX / 2.0f) * cx;
    dys = (dY / 2.0f) * cx;
}

constexpr int MAX_STEPS = AIR_MAX_STEPS;     // the per-image records of the attend / compose / render kernels

// concrete.py:20-27 + air_model.py:385-390: pre-sigmoid sample and z_pres
__device__ __forceinline__ float concrete_noise(float u, float eps = AIR_EPS) {
    return logf(u + eps) - logf((1.0f - u) + eps);
}
__device__ __forceinline__ float concrete_presigmoid(float lo, float u, float T, float eps = AIR_EPS) {
    return (lo + concrete_noise(u, eps)) / T;
}
// concrete.py:35-37 / :39-41: log density of the pre-sigmoid sample y under a binary Concrete with log-odds `lo` and
// temperature T -- one expression for the prior and the posterior of attend_fwd_kernel and for air_concrete_kl_fwd
__device__ __forceinline__ float concrete_log_density(float y, float T, float lo, float eps = AIR_EPS) {
    const float yT = y * T;
    return ((logf(T + eps) - yT) + lo) - 2.0f * logf((1.0f + expf(-yT + lo)) + eps);
}

// ---- compose, the part air_write_fwd and air_render share: one workgroup per image, CF_THREADS threads ----------------
constexpr int CF_THREADS = 1024;

// taps of theta_recon (air_model.py:353-356) for every (step, canvas column / row) and the windows of all N steps of image
// b into LDS: sh_tx / sh_ty [N][C], sh_win [N][w*w]
__device__ __forceinline__ void compose_stage_taps(const float* att, int b, int B, int N, int C, int w, int tid, int nthreads,
                                                   Tap* sh_tx, Tap* sh_ty) {
    for (int it = tid; it < N * C; it += nthreads) {
        const int t = it / C, j = it % C;
        const float* at = att + ((size_t)t * B + b) * AIR_ATT_STRIDE;
        // theta_recon :353-356
        const float s = at[AIR_ATT_S], x = at[AIR_ATT_X], y = at[AIR_ATT_Y];
        const float ia = 1.0f / s, bx = (-x) / s, by = (-y) / s;
        sh_tx[it] = axis_tap(j, C, w, ia, bx);
        sh_ty[it] = axis_tap(j, C, w, ia, by);
    }
}
// element `it` of the N windows of image b ([N][w*w], as sh_win holds them)
__device__ __forceinline__ float compose_window_at(const float* vrec, int b, int B, int w, int it) {
    const int t = it / (w * w);
    return vrec[((size_t)t * B + b) * w * w + (it - t * w * w)];
}
__device__ __forceinline__ void compose_stage_windows(const float* vrec, int b, int B, int N, int w, int first, int nthreads, float* sh_win) {
    for (int it = first; it < N * w * w; it += nthreads) sh_win[it] = compose_window_at(vrec, b, B, w, it);
}
__device__ __forceinline__ void compose_stage(const float* att, const float* vrec, int b, int B, int N,
                                              int C, int w, int tid, int nthreads, Tap* sh_tx, Tap* sh_ty, float* sh_win) {
    compose_stage_taps(att, b, B, N, C, w, tid, nthreads, sh_tx, sh_ty);
    compose_stage_windows(vrec, b, B, N, w, tid, nthreads, sh_win);
}

// running_recon of canvas pixel (i, j) (:552, :429-439): the z-scaled window -> canvas taps of the active steps, summed in
// step order
__device__ __forceinline__ float compose_pixel(const int* sh_act, const float* sh_z, const Tap* sh_tx, const Tap* sh_ty,
                                               const float* sh_win, int N, int C, int w, int i, int j) {
    float R = 0.0f;                                                 // running_recon :552
    for (int t = 0; t < N; ++t) {
        if (!sh_act[t]) continue;                                   // where(active, z*w, 0) :433-439
        const Tap tx = sh_tx[(size_t)t * C + j], ty = sh_ty[(size_t)t * C + i];
        const float* win = sh_win + (size_t)t * w * w;
        const float wr = bilinear4(tx, ty, win[ty.i0 * w + tx.i0], win[ty.i1 * w + tx.i0],
                                   win[ty.i0 * w + tx.i1], win[ty.i1 * w + tx.i1]);
        R = R + sh_z[t] * wr;
    }
    return R;
}

// which step explains canvas pixel (i, j): the terms compose_pixel adds for it (the same operations in the same order),
// compared instead of summed -- the first active step whose term is strictly above `best` and above every earlier one;
// t + 1, or 0 where no term is above `best` (a NaN term never is).  air_segmentation's predicted instance label
__device__ __forceinline__ int compose_label(const int* sh_act, const float* sh_z, const Tap* sh_tx, const Tap* sh_ty,
                                             const float* sh_win, int N, int C, int w, int i, int j, float best) {
    int label = 0;
    for (int t = 0; t < N; ++t) {
        if (!sh_act[t]) continue;
        const Tap tx = sh_tx[(size_t)t * C + j], ty = sh_ty[(size_t)t * C + i];
        const float* win = sh_win + (size_t)t * w * w;
        const float wr = bilinear4(tx, ty, win[ty.i0 * w + tx.i0], win[ty.i1 * w + tx.i0],
                                   win[ty.i0 * w + tx.i1], win[ty.i1 * w + tx.i1]);
        const float c = sh_z[t] * wr;
        if (c > best) { best = c; label = t + 1; }
    }
    return label;
}

// clipped_rec :582 of running_recon R (returned), and the arguments of the two logs of the Bernoulli cross-entropy :586-589
__device__ __forceinline__ float compose_clip(float R, float& p1, float& p0) {
    const float r = fmaxf(fminf(R, 1.0f), 0.0f);
    p1 = r + AIR_EPS; p0 = (1.0f - r) + AIR_EPS;
    return r;
}
// d loss / d running_recon of one pixel (gsc: AIR_DYN_GRAD_SCALE)
__device__ __forceinline__ float compose_dloss(float R, float x, float p1, float p0, float gsc) {
    const bool pass = (R <= 1.0f) && (fminf(R, 1.0f) >= 0.0f);      // Minimum/Maximum grads pass at ties
    return pass ? -gsc * (x / p1 - (1.0f - x) / p0) : 0.0f;
}
// The pixel likelihood of compose, a COMPILE-TIME choice (AIR_LIK_*: the Bernoulli instantiations are the code they were
// before there was a choice): the thread's term of one pixel, d loss / d running_recon of it, and the image's
// reconstruction loss from the block sum of the terms over its D pixels.  g: air_gauss_lik(dyn), unused by Bernoulli.
template <int LIK> struct PixelLik;
template <> struct PixelLik<AIR_LIK_BERNOULLI> {
    static __device__ __forceinline__ float term(float x, float, float p1, float p0) { return x * logf(p1) + (1.0f - x) * logf(p0); }   // :586-589
    static __device__ __forceinline__ float dloss(float R, float, float x, float p1, float p0, float gsc, const AirGaussLik&) {
        return compose_dloss(R, x, p1, p0, gsc);
    }
    static __device__ __forceinline__ float image_loss(float acc, int, const AirGaussLik&) { return -acc; }
};
template <> struct PixelLik<AIR_LIK_GAUSSIAN> {
    static __device__ __forceinline__ float term(float x, float r, float, float) { return air_gauss_term(x, r); }
    static __device__ __forceinline__ float dloss(float R, float r, float x, float, float, float gsc, const AirGaussLik& g) {
        return air_gauss_dloss(R, r, x, gsc, g);
    }
    static __device__ __forceinline__ float image_loss(float acc, int D, const AirGaussLik& g) { return air_gauss_image_loss(acc, D, g); }
};

// air_model.py:443-447 for one element
__device__ __forceinline__ float gauss_kl_term(float plv, float lv, float var, float pv, float mean, float pm) {
    const float d = mean - pm;
    return (((plv - lv) - 1.0f) + var / pv) + (d * d) / pv;
}

// ---- the compose front: what air_write_fwd computes per image, as parts.  write_fwd_kernel runs them on one workgroup
// per image; the compose fold of the write backward (compose_write_bwd_graph_kernel) runs them at the front of every
// workgroup of the image, the workgroup of step 0 (the owner) storing the image's outputs ----------------------------------
// compose's LDS in write_smem's layout, from `base`
struct ComposeLds {
    float* red; float* z; int* act;      // [16]; [MAX_STEPS] z_pres; [MAX_STEPS]
    float* kl; float* rec;               // [MAX_STEPS] VAE KL per step; [MAX_STEPS][4]: mask_prev, KL z, KL scale, KL shift
    Tap* tx; Tap* ty; float* win;        // [N][C] each; [N][w*w]
};
__device__ __forceinline__ ComposeLds compose_lds(float* base, int N, int C, int w) {
    ComposeLds L;
    L.red = base; L.z = base + 16; L.act = reinterpret_cast<int*>(base + 16 + MAX_STEPS);
    L.kl = base + 16 + 2 * MAX_STEPS; L.rec = base + 16 + 3 * MAX_STEPS;
    L.tx = reinterpret_cast<Tap*>(base + 16 + 7 * MAX_STEPS); L.ty = L.tx + (size_t)N * C;
    L.win = reinterpret_cast<float*>(L.ty + (size_t)N * C);
    return L;
}
// VAE KL :479-493 of every step of image b (a public output whether or not the item is still active): one wave per step
template <int NWAVES>
__device__ __forceinline__ void compose_vae_kl(const float* ml_all, const float* dyn, int b, int B, int N, int Z, int lane, int wave,
                                               float* sh_kl) {
    for (int t = wave; t < N; t += NWAVES) {
        const float* ml = ml_all + ((size_t)t * B + b) * 2 * Z;
        const float pv = dyn[AIR_DYN_VAE_PV], pm = dyn[AIR_DYN_VAE_PM], plv = dyn[AIR_DYN_VAE_PLV];
        float klt = 0.0f;
        for (int j = lane; j < Z; j += 64) {
            const float lv = ml[Z + j];
            klt += gauss_kl_term(plv, lv, expf(lv), pv, ml[j], pm);
        }
        klt = air_wave_sum(klt);
        if (lane == 0) sh_kl[t] = 0.5f * klt;
    }
}
// one thread per step fetches its record (six independent loads); one thread then sums from LDS (compose_running_loss) -- as
// a loop of conditional loads on one thread it was a dozen memory round trips in a row
__device__ __forceinline__ void compose_fetch_records(const float* att, int b, int B, int N, int tid, const ComposeLds& L) {
    if (tid < N) {
        const float* at = att + ((size_t)tid * B + b) * AIR_ATT_STRIDE;
        const float zv = at[AIR_ATT_Z], mk = at[AIR_ATT_MASK], mp = at[AIR_ATT_MASK_PREV];
        const float kz = at[AIR_ATT_KL_Z], ks = at[AIR_ATT_KL_SCALE], kh = at[AIR_ATT_KL_SHIFT];
        L.z[tid] = zv;
        L.act[tid] = mk != 0.0f ? 1 : 0;
        L.rec[4 * tid] = mp; L.rec[4 * tid + 1] = kz; L.rec[4 * tid + 2] = ks; L.rec[4 * tid + 3] = kh;
    }
}
// (one thread) the running loss in the reference order: z KL (old mask), scale, shift, VAE KL (new mask) :411-493; the digit
// count; the steps' VAE KL into their records
__device__ __forceinline__ void compose_running_loss(const ComposeLds& L, float* att, int b, int B, int N, float& loss, int& digits) {
    loss = 0.0f;
    digits = 0;
    for (int t = 0; t < N; ++t) {
        const bool mask = L.act[t] != 0;
        loss = loss + (L.rec[4 * t] != 0.0f ? L.rec[4 * t + 1] : 0.0f);
        loss = loss + (mask ? L.rec[4 * t + 2] : 0.0f);
        loss = loss + (mask ? L.rec[4 * t + 3] : 0.0f);
        loss = loss + (mask ? L.kl[t] : 0.0f);
        digits += mask ? 1 : 0;
        att[((size_t)t * B + b) * AIR_ATT_STRIDE + AIR_ATT_KL_VAE] = L.kl[t];
    }
}
// the image pixels of a thread do not depend on anything computed in the launch: on small canvases (<= COMPOSE_XPRE per
// thread) their loads go out with the set-up's -- one memory round trip instead of two
constexpr int COMPOSE_XPRE = 4;
__device__ __forceinline__ bool compose_prefetch_image(const float* images, size_t base, int CC, int tid, float (&xs)[COMPOSE_XPRE]) {
    const bool xpre = CC <= COMPOSE_XPRE * CF_THREADS;
#pragma unroll
    for (int k = 0; k < COMPOSE_XPRE; ++k) { const int p = tid + k * CF_THREADS; xs[k] = images[base + ((xpre && p < CC) ? p : 0)]; }
    return xpre;
}
// canvas + pixel likelihood, pixel by pixel, CF_THREADS threads; returns the thread's part of the likelihood's sum
// (PixelLik<LIK>: the Bernoulli cross-entropy terms, or the squared errors of the Gaussian).
// Compile-time: OUT, who stores the image's outputs (the clipped reconstruction, d loss / d canvas to memory where g_mem is
// given, and the sum) -- 0 nobody, 1 every caller, 2 the callers with `owner`; G_LDS, d loss / d canvas into g_lds as well;
// LIK, the likelihood (glik: its sigma, read by the Gaussian only).
// (Both callers prefetch the image values -- xs / xpre of compose_prefetch_image -- so that is no switch.)
template <int OUT, bool G_LDS, int LIK = AIR_LIK_BERNOULLI>
__device__ __forceinline__ float compose_pixels(const ComposeLds& L, const float* images, size_t base, const float (&xs)[COMPOSE_XPRE],
                                                bool xpre, int N, int C, int w, float gsc, int tid, bool owner,
                                                float* recon, float* g_mem, float* g_lds, const AirGaussLik& glik = AirGaussLik{}) {
    const int CC = C * C;
    const bool store = OUT == 1 || (OUT == 2 && owner);
    float acc = 0.0f;
    const int di = CF_THREADS / C, dj = CF_THREADS % C;
    int i = tid / C, j = tid % C, k = 0;
    for (int p = tid; p < CC; p += CF_THREADS, ++k) {
        float x;
        // (k < COMPOSE_XPRE whenever xpre: a compile-time-indexed pick, written out -- as a loop over a referenced array it
        // was left in scratch memory)
        static_assert(COMPOSE_XPRE == 4, "the pick below");
        if (xpre) x = k == 3 ? xs[3] : k == 2 ? xs[2] : k == 1 ? xs[1] : xs[0];
        else x = images[base + p];
        const float R = compose_pixel(L.act, L.z, L.tx, L.ty, L.win, N, C, w, i, j);
        i += di; j += dj;
        if (j >= C) { j -= C; ++i; }
        float p1, p0;
        const float r = compose_clip(R, p1, p0);                    // clipped_rec :582
        if (G_LDS) g_lds[p] = PixelLik<LIK>::dloss(R, r, x, p1, p0, gsc, glik);
        if (store) {
            acc += PixelLik<LIK>::term(x, r, p1, p0);
            recon[base + p] = r;
            if (g_mem) g_mem[base + p] = PixelLik<LIK>::dloss(R, r, x, p1, p0, gsc, glik);
        }
    }
    return acc;
}

template <typename K>
int ensure_lds(K kernel, size_t bytes) { return air_grant_lds(reinterpret_cast<const void*>(kernel), bytes); }

// ---- dynamic LDS of the sampler launches, in bytes: what the entry points size their launches with, and what air_step_lds
// answers (the host asks; it does not restate these) --------------------------------------------------------------------
// the canvas is staged in LDS only when one prefetch pass covers it (PF * THREADS floats, see the attend kernels)
inline size_t attend_canvas_floats(int C) { return (size_t)C * C <= 10 * (size_t)THREADS ? (size_t)C * C : 0; }
// air_attend_fwd (sh_wout is [7][wout_ld]: the caller's row stride, which may be padded beyond the widest head)
inline size_t attend_smem(int C, int w, int HT, int wout_ld) {
    return (16 + MAX_STEPS + 8 * w + 4 + ((HT + 3) & ~3) + 7 * (size_t)wout_ld + MAX_STEPS * (size_t)HT + attend_canvas_floats(C)) * sizeof(float);
}
// air_attend_bwd
inline size_t attend_bwd_smem(int C, int w) {
    return (24 + 8 * w + w + 4 + attend_canvas_floats(C)) * sizeof(float);
}
// air_write_fwd (with wb_order at least the sort's 16 KB: never the binding term)
inline size_t write_smem(int N, int C, int w) { return (16 + 7 * MAX_STEPS + (size_t)N * (8 * C + (size_t)w * w)) * sizeof(float); }
// air_render
inline size_t render_smem(int N, int C, int w) { return (2 * MAX_STEPS + (size_t)N * (8 * (size_t)C + (size_t)w * w)) * sizeof(float); }
// air_write_bwd, literals 2 and 4: the ONE carve-up of the dynamic LDS, as offsets in floats -- the kernels build their views
// from it and the host sizes the launch with it.  All four taps' terms are resident (allph) when they fit next to a second
// workgroup's share of the LDS; d loss / d canvas is staged (g) only then
struct WbLayout {
    size_t red, acc;     // [128] fin sums / per-wave partials [16][8]; [4] corner accumulators + [4] corner term counts
    size_t tx, ty, t;    // [C] Tap each; [C] linspace
    size_t ci, ri;       // [C] int4 each: per canvas column / row {first, count} of the runs of its two keys
    size_t run, win;     // [4][w][2]: run [lo, hi] of every key of x0 / x1 / y0 / y1; [w*w]
    size_t g, T;         // [C*C] (allph only); [4 or 1][C*C] terms, rectangle-blocked per tap (16-byte aligned)
    size_t floats;       // the whole of it
};
__host__ __device__ inline WbLayout write_bwd_graph_layout(int C, int w, bool allph) {
    const size_t c = (size_t)C, ww = (size_t)w * w, CCp = (c * c + 3) & ~(size_t)3;
    WbLayout L;
    L.red = 0; L.acc = 128; L.tx = 136; L.ty = L.tx + 4 * c; L.t = L.ty + 4 * c;
    L.ci = L.t + ((c + 3) & ~(size_t)3); L.ri = L.ci + 4 * c; L.run = L.ri + 4 * c;
    L.win = L.run + ((8 * (size_t)w + 3) & ~(size_t)3);
    L.g = L.win + ((ww + 3) & ~(size_t)3);
    L.T = L.g + (allph ? CCp : 0);
    L.floats = L.T + (allph ? 4 : 1) * CCp;
    return L;
}
inline size_t write_bwd_graph_smem(int C, int w, bool allph) { return write_bwd_graph_layout(C, w, allph).floats * sizeof(float); }
inline bool write_bwd_graph_allph(int C, int w) { return write_bwd_graph_smem(C, w, true) <= 80 * 1024; }
// air_write_fwd_bwd: compose's scratch (write_smem's layout + the two words handed to the signalling lane) lies over the
// term buffer of the all-taps-resident write backward, which is dead until the term phase
inline size_t compose_fold_floats(int N, int C, int w) { return write_smem(N, C, w) / sizeof(float) + 4; }
inline bool compose_fold_fits(int N, int C, int w) {
    const WbLayout L = write_bwd_graph_layout(C, w, true);
    return compose_fold_floats(N, C, w) <= L.floats - L.T;
}
// air_write_bwd, literal 0
inline size_t write_bwd_smem(int C, int w) { return (64 + 8 * C + C + 8 * w + (size_t)w * w + (size_t)C * w + (size_t)C * C) * sizeof(float); }

}  // namespace
