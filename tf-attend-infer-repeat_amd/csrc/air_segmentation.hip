// Segmentation metrics: ground-truth instance labels of composed scenes, and the predicted instance labels of an inference
// pass scored against a label plane (FG-ARI, best mask IoU per object) -- see the "segmentation metrics" section of
// air_hip.h for the semantics, the order of operations and the summation order.  On the caller's stream, no
// synchronisation, no floating-point atomics:
//   scene_masks_kernel  a workgroup per scene: the digits' metadata into LDS, a label per pixel into an LDS plane, the plane
//                       out 16 bytes at a time (bytes where C * C or the alignment do not allow it).
//   seg_image_kernel    a workgroup of CF_THREADS per image: compose's staging (compose_stage, as render_kernel), a label per
//                       pixel (compose_label: compose_pixel's terms compared instead of summed), the (G + 1) x (T + 1) table
//                       in LDS by integer atomics -- one per distinct cell of a wave, not one per pixel: most of a canvas is
//                       (background, background) -- then the image's scores from the table by a few threads.  Leaves the
//                       image's two fp64 values and its five integer totals in the workspace: a thousand workgroups
//                       adding to the same six words of memory took four times as long as everything else they do.
//   seg_fold_kernel     a workgroup of AIR_LOC_GROUP per accumulator.  A sum: the adjacent pairwise tree over each group of
//                       images, the groups in order, then the incoming accumulator + the batch total.  A count: the
//                       images' integers added up (any order, the same sum), then added to the accumulator.
#include "air_sampler_common.h"

namespace {

constexpr int SEG_GROUP = AIR_LOC_GROUP;                 // the summation group of air_localization, reused
constexpr int SEG_ROWS = AIR_SEG_MAX_DIGITS + 1, SEG_COLS = AIR_SEG_MAX_STEPS + 1;
constexpr int MASK_THREADS = 256;
constexpr int SEG_IMAGE_COUNTS = AIR_SEG_COUNTS - 1;     // per image: every count but IMAGES, at [count - 1]
static_assert(AIR_SEG_IMAGES == 0, "the per-image totals are the counts behind IMAGES");
static_assert(AIR_SEG_MAX_STEPS <= MAX_STEPS, "the records of compose hold MAX_STEPS steps");
static_assert(SEG_GROUP == 256, "the group tree below is written for four waves");

// a label plane of n bytes from LDS to memory: 16 bytes at a time where n and dst allow it
__device__ __forceinline__ void store_plane(const uint8_t* plane /* LDS, 16-byte aligned */, uint8_t* dst, int n, int tid, int nthreads) {
    if ((n & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const uint4* src16 = reinterpret_cast<const uint4*>(plane);
        uint4* dst16 = reinterpret_cast<uint4*>(dst);
        for (int q = tid; q < (n >> 4); q += nthreads) dst16[q] = src16[q];
    } else {
        for (int p = tid; p < n; p += nthreads) dst[p] = plane[p];
    }
}

__global__ __launch_bounds__(MASK_THREADS) void scene_masks_kernel(const air_scene_masks_t a) {
    __shared__ __attribute__((aligned(16))) uint8_t plane[AIR_SCENE_MAX_CANVAS * AIR_SCENE_MAX_CANVAS];
    __shared__ int meta[AIR_SCENE_MAX_DIGITS][8];         // x, y, w, h, x0, y0, glyph index, usable
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = a.C, gd = a.gd, md = a.max_digits, CC = C * C;
    const int n = min(max(a.digits[b], 0), md);
    if (tid < n) {
        const int idx = a.indices[(int64_t)b * md + tid];
        int x0 = 0, y0 = 0, w = 0, h = 0, ok = 0;
        if (idx >= 0 && idx < a.G) {
            const int32_t* cr = a.crops + (int64_t)idx * 4;
            x0 = cr[0]; y0 = cr[1]; w = cr[2]; h = cr[3];
            // (every term is checked against gd before a sum is formed: no overflow)
            ok = x0 >= 0 && y0 >= 0 && w >= 0 && h >= 0 && x0 <= gd && y0 <= gd && w <= gd - x0 && h <= gd - y0;
        }
        int* m = meta[tid];
        m[0] = a.positions[(int64_t)b * 2 * md + 2 * tid]; m[1] = a.positions[(int64_t)b * 2 * md + 2 * tid + 1];
        m[2] = w; m[3] = h; m[4] = x0; m[5] = y0; m[6] = idx; m[7] = ok;
    }
    __syncthreads();
    for (int p = tid; p < CC; p += MASK_THREADS) {
        const int py = p / C, px = p - py * C;
        int label = 0;
        for (int g = 0; g < n; ++g) {
            const int* m = meta[g];
            // 64-bit differences: a position is any int32
            const int64_t dx = (int64_t)px - m[0], dy = (int64_t)py - m[1];
            if (!m[7] || dx < 0 || dx >= m[2] || dy < 0 || dy >= m[3]) continue;
            const float v = a.glyphs[(int64_t)m[6] * gd * gd + (m[5] + (int)dy) * gd + (m[4] + (int)dx)];
            if (v > a.ink_threshold) { label = g + 1; break; }
        }
        plane[p] = (uint8_t)label;
    }
    __syncthreads();
    store_plane(plane, a.mask + (int64_t)b * CC, CC, tid, MASK_THREADS);
}

// dynamic LDS of seg_image_kernel (all of its LDS: the grant of 160 KB of dynamic LDS leaves no room for static arrays):
// the label plane (C * C bytes rounded up to 16), the table and its sums, then render_smem's parts
__host__ __device__ inline size_t seg_plane_bytes(int C) { return ((size_t)C * C + 15) & ~(size_t)15; }
constexpr size_t SEG_TABLE_INTS = SEG_ROWS * SEG_COLS + SEG_ROWS + 2 * SEG_COLS;
constexpr size_t SEG_TABLE_BYTES = (SEG_ROWS * sizeof(double) + SEG_TABLE_INTS * sizeof(int32_t) + 15) & ~(size_t)15;
inline size_t seg_smem(int T, int C, int w) { return render_smem(T, C, w) + seg_plane_bytes(C) + SEG_TABLE_BYTES; }

__global__ __launch_bounds__(CF_THREADS) void seg_image_kernel(const air_segmentation_t a, double* __restrict__ per_image,
                                                               int64_t* __restrict__ per_image_counts) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int i = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int C = a.C, w = a.w, T = a.T, B = a.B, G = a.G, CC = C * C;
    const int W = T + 1, cells = (G + 1) * W;
    // the plane first: 16-byte aligned whatever the sizes behind it
    uint8_t* plane = reinterpret_cast<uint8_t*>(smem);
    double* best_iou = reinterpret_cast<double*>(plane + seg_plane_bytes(C));            // [SEG_ROWS]
    int32_t* tab = reinterpret_cast<int32_t*>(best_iou + SEG_ROWS);       // n[r][c] at r * (T + 1) + c
    int32_t* row = tab + SEG_ROWS * SEG_COLS;                            // [SEG_ROWS]
    int32_t* col_all = row + SEG_ROWS;                                   // [SEG_COLS]
    int32_t* col_fg = col_all + SEG_COLS;                                // [SEG_COLS]
    float* sh_z = smem + (seg_plane_bytes(C) + SEG_TABLE_BYTES) / sizeof(float);         // [MAX_STEPS] z_pres
    int* sh_act = reinterpret_cast<int*>(sh_z + MAX_STEPS);              // [MAX_STEPS]
    Tap* sh_tx = reinterpret_cast<Tap*>(sh_z + 2 * MAX_STEPS);           // [T][C]
    Tap* sh_ty = sh_tx + (size_t)T * C;                                  // [T][C]
    float* sh_win = reinterpret_cast<float*>(sh_ty + (size_t)T * C);     // [T][w*w]

    compose_stage(a.att, a.vrec, i, B, T, C, w, tid, CF_THREADS, sh_tx, sh_ty, sh_win);
    if (tid < T) {
        const float* at = a.att + ((size_t)tid * B + i) * AIR_ATT_STRIDE;
        sh_z[tid] = at[AIR_ATT_Z];
        sh_act[tid] = at[AIR_ATT_MASK] != 0.0f ? 1 : 0;
    }
    for (int j = tid; j < cells; j += CF_THREADS) tab[j] = 0;
    __syncthreads();

    const uint8_t* gt = a.gt_mask + (int64_t)i * CC;
    const int di = CF_THREADS / C, dj = CF_THREADS % C;
    int py = tid / C, px = tid % C;
    for (int p0 = 0; p0 < CC; p0 += CF_THREADS) {         // (uniform trip count: the wave votes below)
        const int p = p0 + tid;
        int cell = -1;
        if (p < CC) {
            const int label = compose_label(sh_act, sh_z, sh_tx, sh_ty, sh_win, T, C, w, py, px, a.pred_threshold);
            const int truth = gt[p];
            plane[p] = (uint8_t)label;
            cell = (truth > G ? 0 : truth) * W + label;
        }
        py += di; px += dj;
        if (px >= C) { px -= C; ++py; }
        // one LDS atomic per distinct cell of the wave (integer: any order, the same counts)
        unsigned long long todo = __ballot(cell >= 0);
        while (todo) {
            const int leader = __ffsll(todo) - 1;
            const int c = __shfl(cell, leader, 64);
            const unsigned long long same = __ballot(cell == c);
            if (lane == leader) atomicAdd(&tab[c], __popcll(same));
            todo &= ~same;
        }
    }
    __syncthreads();

    if (a.pred_mask) store_plane(plane, a.pred_mask + (int64_t)i * CC, CC, tid, CF_THREADS);
    if (a.tables) for (int j = tid; j < cells; j += CF_THREADS) a.tables[(int64_t)i * cells + j] = tab[j];
    if (tid <= G) {
        int32_t s = 0;
        for (int c = 0; c <= T; ++c) s += tab[tid * W + c];
        row[tid] = s;
    }
    if (tid >= 64 && tid - 64 <= T) {                     // (another wave: the two loops run side by side)
        const int c = tid - 64;
        int32_t all = 0;
        for (int r = 0; r <= G; ++r) all += tab[r * W + c];
        col_all[c] = all;
        col_fg[c] = all - tab[c];
    }
    __syncthreads();
    if (tid >= 1 && tid <= G) {
        const int32_t ar = row[tid];
        double v = 0.0;
        if (ar > 0) {
            for (int c = 1; c <= T; ++c) {
                const int32_t n = tab[tid * W + c];
                const double q = (double)n / (double)(ar + col_all[c] - n);
                if (q > v) v = q;
            }
        }
        best_iou[tid] = v;
        if (a.mask_iou) a.mask_iou[(int64_t)i * G + (tid - 1)] = v;
    }
    __syncthreads();
    if (tid == 0) {
        int64_t N = 0, S = 0, A = 0, Bs = 0, missed = 0, claimed = 0;
        int present = 0;
        double miou = 0.0;
        for (int r = 1; r <= G; ++r) {
            const int64_t ar = row[r];
            N += ar;
            A += ar * (ar - 1) / 2;
            missed += tab[r * W];
            if (ar > 0) { ++present; miou = miou + best_iou[r]; }
            for (int c = 0; c <= T; ++c) { const int64_t n = tab[r * W + c]; S += n * (n - 1) / 2; }
        }
        for (int c = 0; c <= T; ++c) { const int64_t bc = col_fg[c]; Bs += bc * (bc - 1) / 2; }
        for (int c = 1; c <= T; ++c) claimed += tab[c];
        const bool scored = N >= 2;
        double ari = 0.0;
        if (scored) {
            const int64_t P = N * (N - 1) / 2;
            const double E = (double)A * (double)Bs / (double)P;
            const double M = ((double)A + (double)Bs) / 2.0;
            ari = (M == E) ? 1.0 : ((double)S - E) / (M - E);
        }
        if (a.ari) a.ari[i] = scored ? ari : __longlong_as_double(0x7FF8000000000000LL);
        per_image[(int64_t)i * AIR_SEG_SUMS + AIR_SEG_ARI] = ari;
        per_image[(int64_t)i * AIR_SEG_SUMS + AIR_SEG_MASK_IOU] = miou;
        int64_t* cnt = per_image_counts + (int64_t)i * SEG_IMAGE_COUNTS;
        cnt[AIR_SEG_SCORED - 1] = scored ? 1 : 0;
        cnt[AIR_SEG_PRESENT - 1] = present;
        cnt[AIR_SEG_FG_PIXELS - 1] = N;
        cnt[AIR_SEG_FG_MISSED - 1] = missed;
        cnt[AIR_SEG_BG_CLAIMED - 1] = claimed;
    }
}

// workgroup j < AIR_SEG_SUMS folds sum j: per group the adjacent pairwise tree (lanes in image order), groups in order,
// incoming last.  Workgroup AIR_SEG_SUMS + c adds up count c (IMAGES: k itself).
__global__ __launch_bounds__(SEG_GROUP) void seg_fold_kernel(const double* __restrict__ per_image, const int64_t* __restrict__ per_image_counts,
                                                             int k, double* __restrict__ sums, int64_t* __restrict__ counts) {
    __shared__ double red[SEG_GROUP / 64];
    __shared__ int64_t ired[SEG_GROUP / 64];
    const int tid = threadIdx.x;
    if (blockIdx.x >= AIR_SEG_SUMS) {
        const int c = blockIdx.x - AIR_SEG_SUMS;
        if (c == AIR_SEG_IMAGES) {
            if (tid == 0) counts[c] += k;
            return;
        }
        int64_t v = 0;
        for (int64_t i = tid; i < k; i += SEG_GROUP) v += per_image_counts[i * SEG_IMAGE_COUNTS + (c - 1)];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v += __shfl_down(v, off, 64);
        if ((tid & 63) == 0) ired[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) counts[c] += (ired[0] + ired[1]) + (ired[2] + ired[3]);
        return;
    }
    const int j = blockIdx.x;
    double total = 0.0;
    for (int64_t g0 = 0; g0 < k; g0 += SEG_GROUP) {
        const int64_t i = g0 + tid;
        double v = i < k ? per_image[i * AIR_SEG_SUMS + j] : 0.0;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v = v + __shfl_down(v, off, 64);
        if ((tid & 63) == 0) red[tid >> 6] = v;
        __syncthreads();
        total = total + ((red[0] + red[1]) + (red[2] + red[3]));
        __syncthreads();
    }
    if (tid == 0) sums[j] = sums[j] + total;
}

int seg_check(int T, int B, int k, int G) {
    if (T < 1 || B < 1 || k < 1 || G < 1 || k > B) return AIR_EINVAL;
    if (T > AIR_SEG_MAX_STEPS || G > AIR_SEG_MAX_DIGITS) return AIR_ELIMIT;
    return 0;
}

}  // namespace

extern "C" int air_scene_masks(const air_scene_masks_t* a, void* stream) {
    if (!a) return AIR_EINVAL;
    if (a->B < 1 || a->G < 1 || a->gd < 1 || a->C < 1 || a->max_digits < 1 || !(a->ink_threshold >= 0.0f)) return AIR_EINVAL;
    if (a->C > AIR_SCENE_MAX_CANVAS || a->gd > AIR_SCENE_MAX_GLYPH || a->max_digits > AIR_SCENE_MAX_DIGITS) return AIR_ELIMIT;
    if (!a->glyphs || !a->crops || !a->digits || !a->indices || !a->positions || !a->mask) return AIR_EINVAL;
    hipLaunchKernelGGL(scene_masks_kernel, dim3(a->B), dim3(MASK_THREADS), 0, air_stream(stream), *a);
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int64_t air_segmentation_workspace_bytes(int T, int B, int k, int G) {
    const int rc = seg_check(T, B, k, G);
    return rc ? rc : (int64_t)k * (AIR_SEG_SUMS + SEG_IMAGE_COUNTS) * 8;
}

extern "C" int air_segmentation(const air_segmentation_t* a, void* workspace, void* stream) {
    if (!a) return AIR_EINVAL;
    const int rc = seg_check(a->T, a->B, a->k, a->G);
    if (rc) return rc;
    if (a->C < 2 || a->w < 2) return AIR_EINVAL;
    if (a->C > AIR_SEG_MAX_CANVAS || a->w > AIR_SEG_MAX_WINDOW) return AIR_ELIMIT;
    const size_t lds = seg_smem(a->T, a->C, a->w);
    if (lds > AIR_LDS_LIMIT) return AIR_ELIMIT;
    if (!(a->pred_threshold >= 0.0f && a->pred_threshold < 1.0f)) return AIR_EINVAL;
    if (!a->att || !a->vrec || !a->gt_mask || !a->counts || !a->sums || !workspace) return AIR_EINVAL;
    const int granted = ensure_lds(seg_image_kernel, lds);
    if (granted) return granted;
    hipStream_t s = air_stream(stream);
    double* per_image = static_cast<double*>(workspace);                                 // [k][AIR_SEG_SUMS], then
    int64_t* per_image_counts = reinterpret_cast<int64_t*>(per_image + (int64_t)a->k * AIR_SEG_SUMS);   // [k][SEG_IMAGE_COUNTS]
    hipLaunchKernelGGL(seg_image_kernel, dim3(a->k), dim3(CF_THREADS), lds, s, *a, per_image, per_image_counts);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(seg_fold_kernel, dim3(AIR_SEG_SUMS + AIR_SEG_COUNTS), dim3(SEG_GROUP), 0, s, per_image, per_image_counts, a->k,
                       a->sums, a->counts);
    AIR_CHECK_LAUNCH();
    return 0;
}
