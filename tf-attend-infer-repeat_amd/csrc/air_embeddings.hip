// Projector export (the reference's embeddings.py:29-131) on the device: see the "projector export" section of air_hip.h
// for the semantics.  Four kernels, all on the caller's stream, no synchronisation, no floating-point atomics:
//   embed_match_kernel    ONE workgroup, a thread per image (images t, t + 128, ... in passes).  The thread walks the
//                         image's ground-truth digits in order and runs the reference's match in fp64, in its order of
//                         operations (the translation unit is built with -ffp-contract=off; the distance goes through
//                         sqrt, not its square: the `<` and `<=` decisions at rounding ties are the reference's).  The step
//                         indices of an image's digits stay in registers, four bits each (T <= 16, G <= 16).  The accepted
//                         counts become row offsets by an exclusive scan in image order: __shfl_up inside a wave, the wave
//                         totals through LDS, the total of a pass carried into the next one.  Thread 0 then advances the
//                         counters; counters[AIR_EMBED_MATCHED] is also the row cursor the next chunk starts from.
//   embed_copy_kernel     a workgroup per (image, digit) slot; an unmatched slot (or one whose row does not fit) exits at
//                         once, the others copy one latent row and one window row.
//   sprite_minmax_kernel  fp64 min / max of 1.0 - window over a grid-stride range, one partial pair per workgroup.
//   sprite_plane_kernel   every workgroup folds the partials (min and max do not depend on the order) and writes its
//                         pixels of the uint8 plane, four per 32-bit store when the row width is a multiple of four.
#include "air_common.h"

namespace {

constexpr int EM_THREADS = 128;                  // embed_match_kernel: images per pass
constexpr int EM_WAVES = EM_THREADS / 64;
constexpr int EC_THREADS = 64;                   // embed_copy_kernel: 196 16-byte pieces of a 28 x 28 window, 3 or 4 per lane
constexpr int SP_THREADS = 256;
constexpr int SP_MAX_PARTIALS = SP_THREADS;      // one partial pair per thread of the plane kernel

// matplotlib's grey colormap as bytes: uint8(linspace(0, 1, 256)[i] * 255), truncating -- linspace is i * (1 / 255) with
// the last entry set to 1.  Not the identity: one below i at 33, 37, 41, ...
struct SpTable { unsigned char g[256]; };
constexpr SpTable sp_make_table() {
    SpTable t{};
    const double step = 1.0 / 255.0;
    for (int i = 0; i < 255; ++i) t.g[i] = (unsigned char)((i * step) * 255.0);
    t.g[255] = 255;
    return t;
}
__device__ const SpTable sp_table = sp_make_table();

__global__ __launch_bounds__(EM_THREADS) void embed_match_kernel(const air_embed_collect_t a, int32_t* __restrict__ rows) {
    __shared__ int32_t wave_total[EM_WAVES];
    __shared__ int32_t sums[2];                  // present, inferred of this chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = a.G;
    const double half = ((double)a.canvas_size - 1.0) / 2.0;          // 24.5 at 50
    if (tid < 2) sums[tid] = 0;
    const int32_t cursor = a.counters[AIR_EMBED_MATCHED];              // stream order: the chunk before this one is done
    int32_t carry = 0;                           // accepted digits of the passes before this one
    __syncthreads();
    for (int base = 0; base < a.k; base += EM_THREADS) {
        const int i = base + tid;
        uint64_t steps = 0;                      // 4 bits per ground-truth digit: the matched step
        uint32_t valid = 0, taken = 0;           // bit g: digit g accepted; bit t: step t taken
        int cnt = 0, ninf = 0;
        if (i < a.k) {
            cnt = min(max(a.gt_count[i], 0), G);
            ninf = min(max(a.run_digits[i], 0), a.T);
            for (int g = 0; g < cnt; ++g) {
                const int32_t* pos = a.gt_positions + ((int64_t)i * G + g) * 2;
                const int32_t* box = a.gt_boxes + ((int64_t)i * G + g) * 2;
                // embeddings.py:41-44: cx = (x + x + w - 1.0) / 2.0, st_cx = cx / 24.5 - 1.0
                const double cx = ((double)(pos[0] + pos[0] + box[0]) - 1.0) / 2.0;
                const double cy = ((double)(pos[1] + pos[1] + box[1]) - 1.0) / 2.0;
                const double x1 = cx / half - 1.0, y1 = cy / half - 1.0;
                int closest = -1;
                double min_distance = 3.0;
                for (int t = 0; t < ninf; ++t) {
                    const float* rec = a.att + ((int64_t)t * a.B + i) * AIR_ATT_STRIDE;
                    const double dx = (double)rec[AIR_ATT_X] - x1, dy = (double)rec[AIR_ATT_Y] - y1;
                    const double dist = sqrt(dx * dx + dy * dy);
                    if (dist < min_distance) { min_distance = dist; closest = t; }
                }
                if (closest >= 0 && min_distance <= a.max_distance && !((taken >> closest) & 1u)) {
                    taken |= 1u << closest;
                    valid |= 1u << g;
                    steps |= (uint64_t)closest << (4 * g);
                }
            }
        }
        const int mine = __popc(valid);
        int incl = mine;                         // inclusive scan of the wave, lanes in image order
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off) incl += up;
        }
        if (lane == 63) wave_total[wave] = incl;
        if (cnt) atomicAdd(&sums[0], cnt);       // integer LDS atomics: any order, the same sum
        if (ninf && i < a.k) atomicAdd(&sums[1], ninf);
        __syncthreads();
        int before = carry, pass_total = 0;
#pragma unroll
        for (int w = 0; w < EM_WAVES; ++w) {
            if (w < wave) before += wave_total[w];
            pass_total += wave_total[w];
        }
        if (i < a.k) {
            int32_t row = cursor + before + (incl - mine);
            for (int g = 0; g < G; ++g) {
                const bool hit = (valid >> g) & 1u;
                a.match[(int64_t)i * G + g] = hit ? (int32_t)((steps >> (4 * g)) & 15u) : -1;
                rows[(int64_t)i * G + g] = hit && row < a.capacity ? row : -1;      // a row that does not fit is not written
                row += hit ? 1 : 0;
            }
        }
        carry += pass_total;
        __syncthreads();                         // wave_total is rewritten by the next pass
    }
    if (tid == 0) {
        a.counters[AIR_EMBED_MATCHED] = cursor + carry;
        a.counters[AIR_EMBED_PRESENT] += sums[0];
        a.counters[AIR_EMBED_INFERRED] += sums[1];
        if (cursor + carry > a.capacity) a.counters[AIR_EMBED_OVERFLOW] = 1;
    }
}

// n floats: 16-byte pieces where both rows are 16-byte aligned, a scalar tail (or all of it) otherwise
__device__ __forceinline__ void em_copy_row(const float* __restrict__ src, float* __restrict__ dst, int n) {
    int done = 0;
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
        const int n4 = n >> 2;
        for (int j = threadIdx.x; j < n4; j += EC_THREADS)
            reinterpret_cast<float4*>(dst)[j] = reinterpret_cast<const float4*>(src)[j];
        done = n4 << 2;
    }
    for (int j = done + threadIdx.x; j < n; j += EC_THREADS) dst[j] = src[j];
}

__global__ __launch_bounds__(EC_THREADS) void embed_copy_kernel(const air_embed_collect_t a, const int32_t* __restrict__ rows) {
    const int slot = blockIdx.x;                 // < k * G
    const int32_t row = rows[slot];
    if (row < 0) return;
    const int i = slot / a.G, t = a.match[slot], d = a.w * a.w;
    const int64_t obj = (int64_t)t * a.B + i;
    em_copy_row(a.ml + obj * (2 * a.Z), a.out_latents + (int64_t)row * a.Z, a.Z);
    em_copy_row(a.vrec + obj * d, a.out_windows + (int64_t)row * d, d);
    if (threadIdx.x == 0) {
        a.out_labels[row] = a.gt_labels[slot];
        a.out_ids[row] = a.gt_ids[slot];
    }
}

__device__ __forceinline__ void sp_block_minmax(double& lo, double& hi, double (*red)[2]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, off, 64));
        hi = fmax(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = lo; red[threadIdx.x >> 6][1] = hi; }
    __syncthreads();
    lo = red[0][0]; hi = red[0][1];
#pragma unroll
    for (int w = 1; w < SP_THREADS / 64; ++w) { lo = fmin(lo, red[w][0]); hi = fmax(hi, red[w][1]); }
}

__global__ __launch_bounds__(SP_THREADS) void sprite_minmax_kernel(const float* __restrict__ windows, int64_t n, int empty_tiles,
                                                                   double* __restrict__ partials) {
    __shared__ double red[SP_THREADS / 64][2];
    double lo = empty_tiles ? 1.0 : (double)__builtin_inff(), hi = empty_tiles ? 1.0 : -(double)__builtin_inff();
    for (int64_t j = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; j < n; j += (int64_t)gridDim.x * SP_THREADS) {
        const double v = 1.0 - (double)windows[j];
        lo = fmin(lo, v); hi = fmax(hi, v);
    }
    sp_block_minmax(lo, hi, red);
    if (threadIdx.x == 0) { partials[2 * blockIdx.x] = lo; partials[2 * blockIdx.x + 1] = hi; }
}

__device__ __forceinline__ uint32_t sp_level(const float* __restrict__ windows, int M, int w, int dim, int y, int x,
                                             double lo, double range, const unsigned char* tab) {
    const int ty = y / w, tx = x / w, i = ty * dim + tx;
    const double v = i < M ? 1.0 - (double)windows[((int64_t)i * w + (y - ty * w)) * w + (x - tx * w)] : 1.0;
    const double nrm = range > 0.0 ? (v - lo) / range : 0.0;
    return tab[min((int)(nrm * 256.0), 255)];
}

__global__ __launch_bounds__(SP_THREADS) void sprite_plane_kernel(const float* __restrict__ windows, int M, int w, int dim,
                                                                  const double* __restrict__ partials, int npartials,
                                                                  unsigned char* __restrict__ plane) {
    __shared__ double red[SP_THREADS / 64][2];
    __shared__ unsigned char tab[256];
    tab[threadIdx.x] = sp_table.g[threadIdx.x];                         // SP_THREADS == 256
    double lo = (double)__builtin_inff(), hi = -(double)__builtin_inff();
    if ((int)threadIdx.x < npartials) { lo = partials[2 * threadIdx.x]; hi = partials[2 * threadIdx.x + 1]; }
    sp_block_minmax(lo, hi, red);                                       // (its barrier also publishes tab)
    const double range = hi - lo;
    const int side = dim * w;
    if ((side & 3) == 0) {                                              // four pixels of one row per 32-bit store
        const int64_t n4 = (int64_t)side * side / 4;
        for (int64_t q = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; q < n4; q += (int64_t)gridDim.x * SP_THREADS) {
            const int y = (int)(4 * q / side), x = (int)(4 * q - (int64_t)y * side);
            uint32_t word = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) word |= sp_level(windows, M, w, dim, y, x + c, lo, range, tab) << (8 * c);
            reinterpret_cast<uint32_t*>(plane)[q] = word;
        }
    } else {
        const int64_t n = (int64_t)side * side;
        for (int64_t q = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; q < n; q += (int64_t)gridDim.x * SP_THREADS) {
            const int y = (int)(q / side), x = (int)(q - (int64_t)y * side);
            plane[q] = (unsigned char)sp_level(windows, M, w, dim, y, x, lo, range, tab);
        }
    }
}

int sp_dim(int M) {                              // ceil(sqrt(M)) in integers
    int dim = 1;
    while ((int64_t)dim * dim < M) ++dim;
    return dim;
}

constexpr int SP_MAX_W = 256, SP_MAX_M = 1 << 22;                       // the plane stays below 2^40 bytes, dim below 2^11

int sp_check(int M, int w) {
    if (M < 1 || w < 1) return AIR_EINVAL;
    if (M > SP_MAX_M || w > SP_MAX_W) return AIR_ELIMIT;
    return 0;
}

int sp_partials(int M, int w) {                  // workgroups of the min / max launch: 2048 elements each, at most 256
    const int64_t n = (int64_t)M * w * w, want = (n + 8 * SP_THREADS - 1) / (8 * SP_THREADS);
    return (int)(want < SP_MAX_PARTIALS ? want : SP_MAX_PARTIALS);
}

int em_check(int T, int B, int k, int G) {
    if (T < 1 || B < 1 || k < 1 || G < 1 || k > B) return AIR_EINVAL;
    if (T > AIR_EMBED_MAX_STEPS || G > AIR_EMBED_MAX_DIGITS) return AIR_ELIMIT;
    return 0;
}

}  // namespace

extern "C" int64_t air_embed_collect_workspace_ints(int T, int B, int k, int G) {
    const int rc = em_check(T, B, k, G);
    return rc ? rc : (int64_t)k * G;
}

extern "C" int air_embed_collect(const air_embed_collect_t* a, void* workspace, void* stream) {
    if (!a) return AIR_EINVAL;
    const int rc = em_check(a->T, a->B, a->k, a->G);
    if (rc) return rc;
    if (!a->att || !a->run_digits || !a->ml || !a->vrec || !a->gt_count || !a->gt_positions || !a->gt_boxes || !a->gt_labels ||
        !a->gt_ids || !a->match || !a->counters || !a->out_latents || !a->out_windows || !a->out_labels || !a->out_ids ||
        !workspace)
        return AIR_EINVAL;
    if (a->Z < 1 || a->w < 1 || a->capacity < 1 || a->canvas_size < 2 || !(a->max_distance > 0.0)) return AIR_EINVAL;
    if (a->w > SP_MAX_W) return AIR_ELIMIT;
    hipStream_t s = air_stream(stream);
    int32_t* rows = static_cast<int32_t*>(workspace);
    hipLaunchKernelGGL(embed_match_kernel, dim3(1), dim3(EM_THREADS), 0, s, *a, rows);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(embed_copy_kernel, dim3(a->k * a->G), dim3(EC_THREADS), 0, s, *a, rows);
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int air_embed_sprite_dim(int M) { return M < 1 ? AIR_EINVAL : (M > SP_MAX_M ? AIR_ELIMIT : sp_dim(M)); }

extern "C" int64_t air_embed_sprites_workspace_doubles(int M, int w) {
    const int rc = sp_check(M, w);
    return rc ? rc : 2 * (int64_t)sp_partials(M, w);
}

extern "C" int air_embed_sprites(const float* windows, int M, int w, void* workspace, uint8_t* plane, void* stream) {
    const int rc = sp_check(M, w);
    if (rc) return rc;
    if (!windows || !workspace || !plane) return AIR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(workspace) & 7) || (reinterpret_cast<uintptr_t>(plane) & 3)) return AIR_EALIGN;
    const int dim = sp_dim(M), parts = sp_partials(M, w);
    const int64_t side = (int64_t)dim * w, pixels = side * side;
    const int64_t items = (side & 3) == 0 ? pixels / 4 : pixels;
    const int64_t want = (items + SP_THREADS - 1) / SP_THREADS;
    const int blocks = (int)(want < 4096 ? want : 4096);
    hipStream_t s = air_stream(stream);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(sprite_minmax_kernel, dim3(parts), dim3(SP_THREADS), 0, s, windows, (int64_t)M * w * w,
                       (int64_t)dim * dim > M ? 1 : 0, partials);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(sprite_plane_kernel, dim3(blocks), dim3(SP_THREADS), 0, s, windows, M, w, dim, partials, parts, plane);
    AIR_CHECK_LAUNCH();
    return 0;
}
