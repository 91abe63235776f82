// Importance-weighted evaluation bound: the log-weights of one sampled pass, and the fold of K of them into the bound, the
// effective sample size and the count posterior -- see the "importance-weighted evaluation bound" section of air_hip.h for
// the semantics, the order of operations and the summation order.  Three kernels on the caller's stream, no
// synchronisation, no floating-point atomics:
//   iw_logw_kernel   a lane per (image, step), IW_IMAGES images x AIR_MAX_STEPS steps in a workgroup.  A lane runs the Z loop
//                    of its step alone (the what-sum is sequential) and leaves the step's four values in LDS; the lane of
//                    step 0 then adds the steps of its image in order.  Every gate is a select.
//   iw_image_kernel  a thread per image, workgroups of AIR_LOC_GROUP.  Registers only: the count posterior is taken count by
//                    count (c outer, samples inner, exp recomputed: the same argument, the same bits) instead of being kept
//                    in a table.  The four fp64 sums of the group are folded by air_localization's adjacent pairwise tree
//                    into one partial quadruple per group; the integer counts go through an LDS table and 64-bit atomics.
//   iw_fold_kernel   four threads: the partials in group order, then the incoming accumulator + the batch total.
#include "air_common.h"

namespace {

constexpr int IW_STEPS = AIR_MAX_STEPS;
constexpr int IW_IMAGES = 16;                       // images of a logw workgroup
constexpr int IW_LOGW_THREADS = IW_IMAGES * IW_STEPS;
constexpr int IW_THREADS = AIR_LOC_GROUP;
constexpr int IW_WAVES = IW_THREADS / 64;
constexpr int IW_MAX_COUNTS = AIR_IW_COUNTS + (AIR_MAX_STEPS + 1) * (AIR_MAX_STEPS + 1);
static_assert(IW_WAVES == 4, "the group tree below is written for four waves");
static_assert(IW_LOGW_THREADS == 256, "a logw workgroup is four waves");

__device__ __forceinline__ double iw_lr(double z, double eps, double lv, double pm, double pv, double plv) {
    return 0.5 * ((((z - pm) * (z - pm)) / pv + plv) - eps * eps - lv);
}

__global__ __launch_bounds__(IW_LOGW_THREADS) void iw_logw_kernel(const air_importance_t a, int sample) {
    __shared__ double part[IW_IMAGES][IW_STEPS][4];             // a_t, gated scale_t, shift_t, what_t
    const int t = threadIdx.x % IW_STEPS, il = threadIdx.x / IW_STEPS;
    const int i = blockIdx.x * IW_IMAGES + il;
    const int T = a.T, B = a.B, Z = a.Z, ldz = a.ldz ? a.ldz : a.Z;
    const bool live = i < a.k && t < T;
    if (live) {
        const int64_t r = (int64_t)t * B + i;
        const float* rec = a.att + r * AIR_ATT_STRIDE;
        const float* o7 = a.out7 + r * AIR_OUT_STRIDE;
        const double scale = iw_lr((double)rec[AIR_ATT_S], (double)a.eps_scale[r], (double)o7[1], (double)a.dyn[AIR_DYN_SCALE_PM],
                                   (double)a.dyn[AIR_DYN_SCALE_PV], (double)a.dyn[AIR_DYN_SCALE_PLV]);
        const double hm = (double)a.dyn[AIR_DYN_SHIFT_PM], hv = (double)a.dyn[AIR_DYN_SHIFT_PV], hl = (double)a.dyn[AIR_DYN_SHIFT_PLV];
        const double shift = iw_lr((double)rec[AIR_ATT_X], (double)a.eps_shift[2 * r], (double)o7[4], hm, hv, hl) +
                             iw_lr((double)rec[AIR_ATT_Y], (double)a.eps_shift[2 * r + 1], (double)o7[5], hm, hv, hl);
        const double vm = (double)a.dyn[AIR_DYN_VAE_PM], vv = (double)a.dyn[AIR_DYN_VAE_PV], vl = (double)a.dyn[AIR_DYN_VAE_PLV];
        const float* zr = a.z + r * ldz;
        const float* er = a.eps_z + r * Z;
        const float* lr = a.ml + r * 2 * Z + Z;
        double what = 0.0;
        for (int j = 0; j < Z; ++j) what = what + iw_lr((double)zr[j], (double)er[j], (double)lr[j], vm, vv, vl);
        const bool on = rec[AIR_ATT_MASK] != 0.0f;
        part[il][t][0] = rec[AIR_ATT_MASK_PREV] != 0.0f ? (double)rec[AIR_ATT_KL_Z] : 0.0;
        part[il][t][1] = on ? scale : 0.0;
        part[il][t][2] = on ? shift : 0.0;
        part[il][t][3] = on ? what : 0.0;
    }
    __syncthreads();
    if (!live || t != 0) return;
    const double rl = (double)a.rec_loss[i];
    double loss = rl, s_z = 0.0, s_scale = 0.0, s_shift = 0.0, s_what = 0.0;
    for (int u = 0; u < T; ++u) {
        const double* p = part[il][u];
        loss = loss + (p[0] + ((p[1] + p[2]) + p[3]));          // (a closed gate left three +0.0: b_t is +0.0)
        s_z = s_z + p[0]; s_scale = s_scale + p[1]; s_shift = s_shift + p[2]; s_what = s_what + p[3];
    }
    const int64_t at = (int64_t)sample * B + i;
    a.logw[at] = -loss;
    a.digits[at] = a.run_digits[i];
    if (a.terms) {
        double* o = a.terms + at * AIR_IW_TERMS;
        o[AIR_IW_TERM_REC] = rl; o[AIR_IW_TERM_Z_PRES] = s_z; o[AIR_IW_TERM_SCALE] = s_scale;
        o[AIR_IW_TERM_SHIFT] = s_shift; o[AIR_IW_TERM_WHAT] = s_what;
    }
}

// adjacent pairwise tree over the 256 values of the group, lanes in image order; thread 0 ends with the total
__device__ __forceinline__ double iw_group_tree(double v, double* red /* [IW_WAVES] */) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ bool iw_finite(double v) { return v - v == 0.0; }

__global__ __launch_bounds__(IW_THREADS) void iw_image_kernel(const air_importance_fold_t a, double* __restrict__ partials) {
    __shared__ int32_t tally[IW_MAX_COUNTS];
    __shared__ double red[AIR_IW_SUMS][IW_WAVES];
    const int tid = threadIdx.x;
    const int T = a.T, K = a.K;
    const int ncounts = AIR_IW_COUNTS + (T + 1) * (T + 1);
    for (int j = tid; j < ncounts; j += IW_THREADS) tally[j] = 0;
    __syncthreads();

    const int i = blockIdx.x * IW_THREADS + tid;
    double v_bound = 0.0, v_elbo = 0.0, v_ess = 0.0, v_entropy = 0.0;
    if (i < a.k) {
        const double* lw = a.logw + i;
        const int32_t* dg = a.digits + i;
        const int64_t B = a.B;
        double m = lw[0];
        for (int s = 1; s < K; ++s) {
            const double l = lw[s * B];
            if (l > m || l != l) m = l;
        }
        atomicAdd(&tally[AIR_IW_IMAGES], 1);                     // integer LDS atomics: any order, the same sums
        if (!iw_finite(m)) {
            atomicAdd(&tally[AIR_IW_DEGENERATE], 1);
            if (a.bound) a.bound[i] = __longlong_as_double(0x7ff8000000000000LL);
            if (a.ess) a.ess[i] = __longlong_as_double(0x7ff8000000000000LL);
            if (a.map) a.map[i] = -1;
        } else {
            const double Kd = (double)K;
            const int d0 = min(max(dg[0], 0), T);
            double S = 0.0, S2 = 0.0, L = 0.0;
            int split = 0;
            for (int s = 0; s < K; ++s) {
                const double l = lw[s * B];
                const double e = exp(l - m);
                S = S + e;
                S2 = S2 + e * e;
                L = L + l;
                split |= min(max(dg[s * B], 0), T) != d0;
            }
            const double bound = m + log(S / Kd);
            const double ess = (S * S) / S2;
            double best = 0.0, ent = 0.0;
            int map = 0;
            for (int c = 0; c <= T; ++c) {
                double W = 0.0;
                for (int s = 0; s < K; ++s)
                    if (min(max(dg[s * B], 0), T) == c) W = W + exp(lw[s * B] - m);
                if (c == 0 || W > best) { best = W; map = c; }
                if (W != 0.0) { const double p = W / S; ent = ent + p * log(p); }
            }
            v_bound = bound; v_elbo = L / Kd; v_ess = ess; v_entropy = -ent;
            if (a.bound) a.bound[i] = bound;
            if (a.ess) a.ess[i] = ess;
            if (a.map) a.map[i] = map;
            atomicAdd(&tally[AIR_IW_SCORED], 1);
            if (split) atomicAdd(&tally[AIR_IW_SPLIT], 1);
            if (a.targets) {
                const int g = min(max(a.targets[i], 0), T);
                if (g == map) atomicAdd(&tally[AIR_IW_MAP_CORRECT], 1);
                atomicAdd(&tally[AIR_IW_COUNTS + g * (T + 1) + map], 1);
            }
        }
    }
    const double g_bound = iw_group_tree(v_bound, red[AIR_IW_BOUND]);
    const double g_elbo = iw_group_tree(v_elbo, red[AIR_IW_ELBO]);
    const double g_ess = iw_group_tree(v_ess, red[AIR_IW_ESS]);
    const double g_entropy = iw_group_tree(v_entropy, red[AIR_IW_ENTROPY]);   // (its barrier also closes the tally)
    if (tid == 0) {
        double* out = partials + (int64_t)blockIdx.x * AIR_IW_SUMS;
        out[AIR_IW_BOUND] = g_bound; out[AIR_IW_ELBO] = g_elbo; out[AIR_IW_ESS] = g_ess; out[AIR_IW_ENTROPY] = g_entropy;
    }
    for (int j = tid; j < ncounts; j += IW_THREADS) {
        const int32_t v = tally[j];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + j, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(64) void iw_fold_kernel(const double* __restrict__ partials, int groups, double* __restrict__ sums) {
    const int j = threadIdx.x;
    if (j >= AIR_IW_SUMS) return;
    double total = 0.0;
    for (int g = 0; g < groups; ++g) total = total + partials[(int64_t)g * AIR_IW_SUMS + j];
    sums[j] = sums[j] + total;
}

int iw_fold_check(int T, int B, int k, int K) {
    if (T < 1 || B < 1 || k < 1 || K < 1 || k > B) return AIR_EINVAL;
    if (T > AIR_MAX_STEPS || K > AIR_IW_MAX_SAMPLES) return AIR_ELIMIT;
    return 0;
}

int iw_groups(int k) { return (int)(((int64_t)k + IW_THREADS - 1) / IW_THREADS); }

}  // namespace

extern "C" int air_importance_logw(const air_importance_t* a, int sample, void* stream) {
    if (!a) return AIR_EINVAL;
    if (a->T < 1 || a->B < 1 || a->k < 1 || a->Z < 1 || a->K < 1 || a->k > a->B) return AIR_EINVAL;
    if ((a->ldz != 0 && a->ldz < a->Z) || sample < 0 || sample >= a->K) return AIR_EINVAL;
    if (a->T > AIR_MAX_STEPS || a->K > AIR_IW_MAX_SAMPLES || a->Z > AIR_IW_MAX_Z) return AIR_ELIMIT;
    if (!a->att || !a->out7 || !a->ml || !a->z || !a->eps_scale || !a->eps_shift || !a->eps_z || !a->rec_loss ||
        !a->run_digits || !a->dyn || !a->logw || !a->digits)
        return AIR_EINVAL;
    const int groups = (int)(((int64_t)a->k + IW_IMAGES - 1) / IW_IMAGES);
    hipLaunchKernelGGL(iw_logw_kernel, dim3(groups), dim3(IW_LOGW_THREADS), 0, air_stream(stream), *a, sample);
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t air_importance_fold_workspace_bytes(int T, int B, int k, int K) {
    const int rc = iw_fold_check(T, B, k, K);
    return rc ? rc : (int64_t)iw_groups(k) * AIR_IW_SUMS * (int64_t)sizeof(double);
}

extern "C" int air_importance_fold(const air_importance_fold_t* a, void* workspace, void* stream) {
    if (!a) return AIR_EINVAL;
    const int rc = iw_fold_check(a->T, a->B, a->k, a->K);
    if (rc) return rc;
    if (!a->logw || !a->digits || !a->counts || !a->sums || !workspace) return AIR_EINVAL;
    hipStream_t s = air_stream(stream);
    const int groups = iw_groups(a->k);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(iw_image_kernel, dim3(groups), dim3(IW_THREADS), 0, s, *a, partials);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(iw_fold_kernel, dim3(1), dim3(64), 0, s, partials, groups, a->sums);
    AIR_CHECK_LAUNCH();
    return 0;
}
