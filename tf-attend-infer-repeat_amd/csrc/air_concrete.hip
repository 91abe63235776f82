// The binary Concrete ops of the reference's air/concrete.py as launches of their own, forward and backward
// (include/air_hip.h, "stand-alone Concrete and VAE pieces").  The train step computes the same expressions inside
// attend_fwd_kernel / attend_bwd_kernel; the sample and the log density are the device functions those kernels call
// (air_sampler_common.h), so a value computed here has the bits of the model's.
#include "air_sampler_common.h"
#include "air_elementwise.h"

namespace {

// concrete.py:4-17
struct SampleFwd {
    const float* lo; const float* u; EwScalar T; float eps; int hard; float* y; float* sig;
    template <int W> __device__ __forceinline__ void run(long i) const {
        float l[W], uu[W], t[W], yv[W], s[W];
        ew_ld<W>(lo, i, l); ew_ld<W>(u, i, uu); ew_lds<W>(T, i, t);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            yv[k] = l[k] + concrete_noise(uu[k], eps);
            s[k] = air_sigmoid(yv[k] / t[k]);
            if (hard) s[k] = rintf(s[k]);                      // tf.round: half to even
        }
        if (y) ew_st<W>(y, i, yv);
        if (sig) ew_st<W>(sig, i, s);
    }
};

// SigmoidGrad (dy * s * (1 - s)), then RealDiv's gradient, then the AddN with what arrives at y itself
struct SampleBwd {
    const float* y; EwScalar T; const float* dy; const float* dsig; float* dlo;
    template <int W> __device__ __forceinline__ void run(long i) const {
        float yv[W], t[W], gy[W], gs[W], out[W];
        ew_ld<W>(y, i, yv); ew_lds<W>(T, i, t); ew_ld0<W>(dy, i, gy); ew_ld0<W>(dsig, i, gs);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float s = air_sigmoid(yv[k] / t[k]);
            out[k] = gy[k] + (gs[k] * (s * (1.0f - s))) / t[k];
        }
        ew_st<W>(dlo, i, out);
    }
};

// concrete.py:20-27
struct PresigmoidFwd {
    const float* lo; const float* u; EwScalar T; float eps; float* y;
    template <int W> __device__ __forceinline__ void run(long i) const {
        float l[W], uu[W], t[W], yv[W];
        ew_ld<W>(lo, i, l); ew_ld<W>(u, i, uu); ew_lds<W>(T, i, t);
#pragma unroll
        for (int k = 0; k < W; ++k) yv[k] = concrete_presigmoid(l[k], uu[k], t[k], eps);
        ew_st<W>(y, i, yv);
    }
};

struct PresigmoidBwd {
    const float* dy; EwScalar T; float* dlo;
    template <int W> __device__ __forceinline__ void run(long i) const {
        float g[W], t[W], out[W];
        ew_ld<W>(dy, i, g); ew_lds<W>(T, i, t);
#pragma unroll
        for (int k = 0; k < W; ++k) out[k] = g[k] / t[k];
        ew_st<W>(dlo, i, out);
    }
};

// concrete.py:30-43
struct KlFwd {
    const float* y; EwScalar plo, pT; const float* qlo; EwScalar qT; float eps; float* kl;
    template <int W> __device__ __forceinline__ void run(long i) const {
        float yv[W], a[W], tp[W], b[W], tq[W], out[W];
        ew_ld<W>(y, i, yv); ew_lds<W>(plo, i, a); ew_lds<W>(pT, i, tp); ew_ld<W>(qlo, i, b); ew_lds<W>(qT, i, tq);
#pragma unroll
        for (int k = 0; k < W; ++k)
            out[k] = concrete_log_density(yv[k], tq[k], b[k], eps) - concrete_log_density(yv[k], tp[k], a[k], eps);
        ew_st<W>(kl, i, out);
    }
};

// d log r / d a = 1 - 2 e / D with e = exp(-y T + a), D = 1 + e + eps (the forward's own e and D);  d log r / d y = -T times it.
// exp overflows to inf for -y T + a > 88.7: the quotient's limit is 1 (e / D -> 1), which inf / inf does not give
__device__ __forceinline__ float concrete_dlogp_da(float y, float T, float a, float eps) {
    const float e = expf(-(y * T) + a);
    const float D = (1.0f + e) + eps;
    const float r = (e > 3.0e38f) ? 1.0f : e / D;
    return 1.0f - 2.0f * r;
}

struct KlBwd {
    const float* g; const float* y; EwScalar plo, pT; const float* qlo; EwScalar qT; float eps;
    float* dy; float* dqlo; float* dplo;
    template <int W> __device__ __forceinline__ void run(long i) const {
        float gv[W], yv[W], a[W], tp[W], b[W], tq[W], o_y[W], o_q[W], o_p[W];
        ew_ld<W>(g, i, gv); ew_ld<W>(y, i, yv); ew_lds<W>(plo, i, a); ew_lds<W>(pT, i, tp);
        ew_ld<W>(qlo, i, b); ew_lds<W>(qT, i, tq);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float dq = concrete_dlogp_da(yv[k], tq[k], b[k], eps);
            const float dp = concrete_dlogp_da(yv[k], tp[k], a[k], eps);
            o_q[k] = gv[k] * dq;
            o_p[k] = -(gv[k] * dp);
            o_y[k] = gv[k] * (tp[k] * dp - tq[k] * dq);
        }
        if (dy) ew_st<W>(dy, i, o_y);
        if (dqlo) ew_st<W>(dqlo, i, o_q);
        if (dplo) ew_st<W>(dplo, i, o_p);
    }
};

}  // namespace

extern "C" int air_concrete_sample_fwd(const float* log_odds, const float* u, const air_scalar_t* temperature, float eps,
                                       int hard, float* y, float* sig_y, int64_t n, void* stream) {
    if (!log_odds || !u || ew_bad(temperature) || (!y && !sig_y) || n < 1) return AIR_EINVAL;
    const bool vec = ew_al16(log_odds) && ew_al16(u) && ew_al16(*temperature) && ew_al16(y) && ew_al16(sig_y);
    return ew_launch(SampleFwd{log_odds, u, ew_scalar(*temperature), eps, hard, y, sig_y}, n, vec, stream);
}

extern "C" int air_concrete_sample_bwd(const float* y, const air_scalar_t* temperature, const float* d_y,
                                       const float* d_sig_y, float* d_log_odds, int64_t n, void* stream) {
    if (!y || ew_bad(temperature) || (!d_y && !d_sig_y) || !d_log_odds || n < 1) return AIR_EINVAL;
    const bool vec = ew_al16(y) && ew_al16(*temperature) && ew_al16(d_y) && ew_al16(d_sig_y) && ew_al16(d_log_odds);
    return ew_launch(SampleBwd{y, ew_scalar(*temperature), d_y, d_sig_y, d_log_odds}, n, vec, stream);
}

extern "C" int air_concrete_presigmoid_fwd(const float* log_odds, const float* u, const air_scalar_t* temperature, float eps,
                                           float* y, int64_t n, void* stream) {
    if (!log_odds || !u || ew_bad(temperature) || !y || n < 1) return AIR_EINVAL;
    const bool vec = ew_al16(log_odds) && ew_al16(u) && ew_al16(*temperature) && ew_al16(y);
    return ew_launch(PresigmoidFwd{log_odds, u, ew_scalar(*temperature), eps, y}, n, vec, stream);
}

extern "C" int air_concrete_presigmoid_bwd(const float* d_y, const air_scalar_t* temperature, float* d_log_odds, int64_t n,
                                           void* stream) {
    if (!d_y || ew_bad(temperature) || !d_log_odds || n < 1) return AIR_EINVAL;
    const bool vec = ew_al16(d_y) && ew_al16(*temperature) && ew_al16(d_log_odds);
    return ew_launch(PresigmoidBwd{d_y, ew_scalar(*temperature), d_log_odds}, n, vec, stream);
}

extern "C" int air_concrete_kl_fwd(const float* y, const air_scalar_t* prior_log_odds, const air_scalar_t* prior_temperature,
                                   const float* posterior_log_odds, const air_scalar_t* posterior_temperature, float eps,
                                   float* kl, int64_t n, void* stream) {
    if (!y || ew_bad(prior_log_odds) || ew_bad(prior_temperature) || !posterior_log_odds || ew_bad(posterior_temperature) ||
        !kl || n < 1) return AIR_EINVAL;
    const bool vec = ew_al16(y) && ew_al16(*prior_log_odds) && ew_al16(*prior_temperature) && ew_al16(posterior_log_odds) &&
                     ew_al16(*posterior_temperature) && ew_al16(kl);
    return ew_launch(KlFwd{y, ew_scalar(*prior_log_odds), ew_scalar(*prior_temperature), posterior_log_odds,
                           ew_scalar(*posterior_temperature), eps, kl}, n, vec, stream);
}

extern "C" int air_concrete_kl_bwd(const float* d_kl, const float* y, const air_scalar_t* prior_log_odds,
                                   const air_scalar_t* prior_temperature, const float* posterior_log_odds,
                                   const air_scalar_t* posterior_temperature, float eps, float* d_y,
                                   float* d_posterior_log_odds, float* d_prior_log_odds, int64_t n, void* stream) {
    if (!d_kl || !y || ew_bad(prior_log_odds) || ew_bad(prior_temperature) || !posterior_log_odds ||
        ew_bad(posterior_temperature) || (!d_y && !d_posterior_log_odds && !d_prior_log_odds) || n < 1) return AIR_EINVAL;
    // a gradient per element exists only for a per-element prior
    if (d_prior_log_odds && !(prior_log_odds->ptr && prior_log_odds->stride == 1)) return AIR_EINVAL;
    const bool vec = ew_al16(d_kl) && ew_al16(y) && ew_al16(*prior_log_odds) && ew_al16(*prior_temperature) &&
                     ew_al16(posterior_log_odds) && ew_al16(*posterior_temperature) && ew_al16(d_y) &&
                     ew_al16(d_posterior_log_odds) && ew_al16(d_prior_log_odds);
    return ew_launch(KlBwd{d_kl, y, ew_scalar(*prior_log_odds), ew_scalar(*prior_temperature), posterior_log_odds,
                           ew_scalar(*posterior_temperature), eps, d_y, d_posterior_log_odds, d_prior_log_odds}, n, vec, stream);
}
