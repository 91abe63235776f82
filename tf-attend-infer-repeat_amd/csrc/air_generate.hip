// Generation: scenes from the priors, or from latents the caller supplies -- the generative half of the loop body
// (air_model.py:288-439, 582; vae.py:26-41) with the posterior heads replaced by the priors.  Three small launches
// around the decoder GEMMs (air_gemm with the forward's descriptors):
//   air_philox_fill    noise keyed by (seed, call counter) -- no schedules, no global_step
//   air_scene_records  the att records of all (step, image) pairs + the latents the first generative GEMM reads
//   air_render         compose without a loss: the staging and per-pixel code of write_fwd_kernel (air_sampler_common.h),
//                      so the canvas equals air_write_fwd's on the same records bit for bit
#include "air_sampler_common.h"
#include "air_philox.h"

namespace {

__global__ __launch_bounds__(THREADS) void philox_fill_kernel(float* normals, long n_normal, float* uniforms, long n_uniform,
                                                              uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    const long quads_n = (n_normal + 3) / 4, quads_u = (n_uniform + 3) / 4;
    for (long q = (long)blockIdx.x * THREADS + threadIdx.x; q < quads_n + quads_u; q += (long)gridDim.x * THREADS)
        air_philox_quad(q, quads_n, c2, c3, k0, k1, normals, n_normal, uniforms, n_uniform);
}

// ---------------------------------------------------------------------------
// records: thread g < B walks image g through its N steps (the stopping sum is the only cross-step dependence: the same
// op sequence as attend_fwd_kernel's, S = S + (1 - z) in step order); every thread also takes its share of the latents.
// A record is four 16-byte stores; the latents are a plain element-wise stream (Z = 50: rows are not 16-byte aligned).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(THREADS) void scene_records_kernel(air_scene_records_t a)
{
    const long gid = (long)blockIdx.x * THREADS + threadIdx.x, nthreads = (long)gridDim.x * THREADS;
    const int B = a.B, N = a.N, Z = a.Z, ldz = a.ldz;
    const float* dyn = a.dyn;
    const bool given = a.given != 0;

    if (gid < B) {
        const int b = (int)gid;
        const float T = dyn[AIR_DYN_TEMPERATURE], thr = dyn[AIR_DYN_STOP_THRESHOLD], plo = dyn[AIR_DYN_PRIOR_LOG_ODDS];
        const float s_pm = dyn[AIR_DYN_SCALE_PM], s_sd = sqrtf(dyn[AIR_DYN_SCALE_PV]);
        const float h_pm = dyn[AIR_DYN_SHIFT_PM], h_sd = sqrtf(dyn[AIR_DYN_SHIFT_PV]);
        // the sources of all steps first (independent loads: one memory round trip), then the sequential part
        float in_s[MAX_STEPS], in_x[MAX_STEPS], in_y[MAX_STEPS], in_p[MAX_STEPS];
#pragma unroll
        for (int t = 0; t < MAX_STEPS; ++t) {
            const size_t row = (size_t)(t < N ? t : 0) * B + b;
            in_s[t] = a.scale_src[row]; in_x[t] = a.shift_src[2 * row]; in_y[t] = a.shift_src[2 * row + 1]; in_p[t] = a.pres_src[row];
        }
        float S = 0.0f;                                             // stopping_sum :550
#pragma unroll
        for (int t = 0; t < MAX_STEPS; ++t) {
            if (t < N) {
                float s, x, y, z, ypre = 0.0f;
                if (given) { s = in_s[t]; x = in_x[t]; y = in_y[t]; z = in_p[t]; }
                else {
                    s = air_sigmoid(s_pm + in_s[t] * s_sd);         // :300-303 on the prior
                    x = tanhf(h_pm + in_x[t] * h_sd);               // :317-320
                    y = tanhf(h_pm + in_y[t] * h_sd);
                    ypre = concrete_presigmoid(plo, in_p[t], T);    // concrete.py:20-27 on the prior log-odds
                    z = rintf(air_sigmoid(ypre));                   // tf.round (half-to-even) :389-390
                }
                const bool mask_prev = S < thr;                     // :409-427
                S = S + (1.0f - z);
                const bool mask = S < thr;
                float4* at = reinterpret_cast<float4*>(a.att + ((size_t)t * B + b) * AIR_ATT_STRIDE);
                at[0] = make_float4(s, x, y, ypre);                                     // S, X, Y, ZPRE
                at[1] = make_float4(z, 0.0f, 0.0f, 0.0f);                               // Z, ZPROB, KL_Z, KL_SCALE
                at[2] = make_float4(0.0f, 0.0f, mask_prev ? 1.0f : 0.0f, mask ? 1.0f : 0.0f);   // KL_SHIFT, KL_VAE, MASK_PREV, MASK
                at[3] = make_float4(1.0f / s, (-x) / s, (-y) / s, 0.0f);                // theta_recon :353-356
            }
        }
    }

    const float z_pm = dyn[AIR_DYN_VAE_PM], z_sd = sqrtf(dyn[AIR_DYN_VAE_PV]);
    const long total = (long)N * B * ldz;
    for (long e = gid; e < total; e += nthreads) {
        const long row = e / ldz;
        const int j = (int)(e - row * ldz);
        float v = 0.0f;
        if (j < Z) {
            const float src = a.z_src[row * Z + j];
            v = given ? src : z_pm + src * z_sd;                    // vae.py:22-24 on the prior
        }
        a.z[e] = v;
        if (a.z16) a.z16[e] = air_bf16_of(v);
    }
}

// ---------------------------------------------------------------------------
// render: one workgroup of CF_THREADS threads per image, the taps and windows of all N steps staged in LDS as in
// write_fwd_kernel; its phase B without the image read, the loss and the gradient.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(CF_THREADS) void render_kernel(air_render_t a)
{
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = a.C, w = a.w, N = a.N, B = a.B;
    float* sh_z = smem;                                                  // [MAX_STEPS] z_pres
    int* sh_act = reinterpret_cast<int*>(smem + MAX_STEPS);              // [MAX_STEPS]
    Tap* sh_tx = reinterpret_cast<Tap*>(smem + 2 * MAX_STEPS);           // [N][C]
    Tap* sh_ty = sh_tx + (size_t)N * C;                                  // [N][C]
    float* sh_win = reinterpret_cast<float*>(sh_ty + (size_t)N * C);     // [N][w*w]
    const size_t base = (size_t)b * C * C;
    const int CC = C * C;

    compose_stage(a.att, a.vrec, b, B, N, C, w, tid, CF_THREADS, sh_tx, sh_ty, sh_win);
    if (tid < N) {
        const float* at = a.att + ((size_t)tid * B + b) * AIR_ATT_STRIDE;
        sh_z[tid] = at[AIR_ATT_Z];
        sh_act[tid] = at[AIR_ATT_MASK] != 0.0f ? 1 : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int digits = 0;                                                  // running_digits :427
        for (int t = 0; t < N; ++t) digits += sh_act[t];
        a.num_digits[b] = digits;
    }
    const int di = CF_THREADS / C, dj = CF_THREADS % C;
    int i = tid / C, j = tid % C;
    for (int p = tid; p < CC; p += CF_THREADS) {
        const float R = compose_pixel(sh_act, sh_z, sh_tx, sh_ty, sh_win, N, C, w, i, j);
        i += di; j += dj;
        if (j >= C) { j -= C; ++i; }
        a.canvas[base + p] = fmaxf(fminf(R, 1.0f), 0.0f);               // clipped_rec :582
    }
}

}  // namespace

extern "C" int air_philox_fill(float* normals, int64_t n_normal, float* uniforms, int64_t n_uniform,
                               uint64_t seed, uint64_t call, void* stream) {
    if (n_normal < 0 || n_uniform < 0 || n_normal + n_uniform <= 0) return AIR_EINVAL;
    if ((n_normal > 0 && !normals) || (n_uniform > 0 && !uniforms)) return AIR_EINVAL;
    const long quads = (long)((n_normal + 3) / 4 + (n_uniform + 3) / 4);
    long blocks = (quads + THREADS - 1) / THREADS;
    if (blocks > 2048) blocks = 2048;
    // counter words 2, 3: the call number under a salt of its own ("GEN1"; the step prologue's is "AIR!")
    hipLaunchKernelGGL(philox_fill_kernel, dim3((int)blocks), dim3(THREADS), 0, air_stream(stream),
                       normals, (long)n_normal, uniforms, (long)n_uniform,
                       (uint32_t)(call & 0xffffffffu), 0x47454E31u + (uint32_t)(call >> 32),
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int air_scene_records(const air_scene_records_t* a, void* stream) {
    if (!a || !a->scale_src || !a->shift_src || !a->z_src || !a->pres_src || !a->dyn || !a->att || !a->z) return AIR_EINVAL;
    if (a->B <= 0 || a->N <= 0 || a->Z <= 0 || a->ldz < a->Z) return AIR_EINVAL;
    if (a->N > MAX_STEPS) return AIR_ELIMIT;
    if ((((uintptr_t)a->att) & 15) != 0) return AIR_EALIGN;
    const long total = (long)a->N * a->B * a->ldz;
    long blocks = ((total > a->B ? total : a->B) + THREADS - 1) / THREADS;
    if (blocks > 2048) blocks = 2048;
    if (blocks * THREADS < a->B) return AIR_ELIMIT;                 // (every image needs a thread of its own)
    hipLaunchKernelGGL(scene_records_kernel, dim3((int)blocks), dim3(THREADS), 0, air_stream(stream), *a);
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int air_render(const air_render_t* a, void* stream) {
    if (!a || !a->vrec || !a->att || !a->canvas || !a->num_digits) return AIR_EINVAL;
    if (a->B <= 0 || a->N <= 0 || a->C < 2 || a->w < 2) return AIR_EINVAL;
    if (a->N > MAX_STEPS) return AIR_ELIMIT;
    const size_t lds = render_smem(a->N, a->C, a->w);
    const int rc = ensure_lds(render_kernel, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(render_kernel, dim3(a->B), dim3(CF_THREADS), lds, air_stream(stream), *a);
    AIR_CHECK_LAUNCH();
    return 0;
}
