// Localisation metrics: the attention boxes of an inference pass scored against ground-truth boxes -- see the "localisation
// metrics" section of air_hip.h for the semantics, the order of operations and the summation order.  Two kernels on the
// caller's stream, no synchronisation, no floating-point atomics:
//   loc_match_kernel  a thread per image, workgroups of AIR_LOC_GROUP.  Per-thread state is registers only (DESIGN.md section
//                     9): the used digits and objects are 16-bit masks, the object of every digit four bits of one 64-bit
//                     word, and a pair's IoU is recomputed inside the greedy scan (at most 16 rounds x 256 pairs) instead of
//                     being kept in a G x T matrix.  The three fp64 sums of the group are folded by the adjacent pairwise
//                     tree (__shfl_down inside a wave, the four wave totals through LDS) into one partial triple per
//                     group; the integer counts go through an LDS table and 64-bit integer atomics.
//   loc_fold_kernel   three threads: the partials in group order, then the incoming accumulator + the batch total.
#include "air_common.h"

namespace {

constexpr int LOC_THREADS = AIR_LOC_GROUP;
constexpr int LOC_WAVES = LOC_THREADS / 64;
constexpr int LOC_MAX_COUNTS = AIR_LOC_COUNTS + (AIR_LOC_MAX_DIGITS + 1) * (AIR_LOC_MAX_STEPS + 1);
static_assert(LOC_WAVES == 4, "the group tree below is written for four waves");

struct LocBox { double l, r, t, b; };
struct LocPair { double iou, cover; };

__device__ __forceinline__ double loc_clip(double v, double C) { return v < 0.0 ? 0.0 : (v > C ? C : v); }
__device__ __forceinline__ double loc_min(double a, double b) { return a < b ? a : b; }
__device__ __forceinline__ double loc_max(double a, double b) { return a > b ? a : b; }

__device__ __forceinline__ LocBox loc_inferred_box(const float* __restrict__ rec, double q, double C) {
    const double s = (double)rec[AIR_ATT_S], x = (double)rec[AIR_ATT_X], y = (double)rec[AIR_ATT_Y];
    LocBox o;
    o.l = loc_clip((x - s + 1.0) * q, C);
    o.r = loc_clip((x + s + 1.0) * q + 1.0, C);
    o.t = loc_clip((y - s + 1.0) * q, C);
    o.b = loc_clip((y + s + 1.0) * q + 1.0, C);
    return o;
}

__device__ __forceinline__ LocPair loc_pair(const LocBox& o, const LocBox& d, double a_gt) {
    LocPair p{0.0, 0.0};
    const double iw = loc_min(o.r, d.r) - loc_max(o.l, d.l);
    const double ih = loc_min(o.b, d.b) - loc_max(o.t, d.t);
    if (iw > 0.0 && ih > 0.0) {
        const double inter = iw * ih;
        const double a_inf = (o.r - o.l) * (o.b - o.t);
        const double uni = a_inf + a_gt - inter;
        if (uni > 0.0) { p.iou = inter / uni; p.cover = inter / a_gt; }
    }
    return p;
}

// adjacent pairwise tree over the 256 values of the group, lanes in image order; thread 0 ends with the total
__device__ __forceinline__ double loc_group_tree(double v, double* red /* [LOC_WAVES] */) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(LOC_THREADS) void loc_match_kernel(const air_localization_t a, double* __restrict__ partials) {
    __shared__ int32_t tally[LOC_MAX_COUNTS];
    __shared__ double red[AIR_LOC_SUMS][LOC_WAVES];
    const int tid = threadIdx.x;
    const int T = a.T, G = a.G;
    const int ncounts = AIR_LOC_COUNTS + (G + 1) * (T + 1);
    for (int j = tid; j < ncounts; j += LOC_THREADS) tally[j] = 0;
    __syncthreads();

    const int i = blockIdx.x * LOC_THREADS + tid;
    const double C = (double)a.canvas_size;
    const double q = (C - 1.001) / 2.0;
    const double half = (C - 1.0) / 2.0;
    double s_iou = 0.0, s_cover = 0.0, s_dist = 0.0;
    if (i < a.k) {
        const int cnt = min(max(a.gt_count[i], 0), G);
        const int ninf = min(max(a.run_digits[i], 0), T);
        const int32_t* pos = a.gt_positions + (int64_t)i * G * 2;
        const int32_t* box = a.gt_boxes + (int64_t)i * G * 2;
        const float* rec0 = a.att + (int64_t)i * AIR_ATT_STRIDE;
        const int64_t rec_step = (int64_t)a.B * AIR_ATT_STRIDE;
        uint64_t steps = 0;                      // 4 bits per digit: the object taken with it
        uint32_t used_g = 0, used_t = 0;
        const int rounds = min(cnt, ninf);
        for (int r = 0; r < rounds; ++r) {
            double best = 0.0;
            int bg = -1, bt = -1;
            for (int g = 0; g < cnt; ++g) {
                if ((used_g >> g) & 1u) continue;
                const double x = (double)pos[2 * g], y = (double)pos[2 * g + 1];
                const double w = (double)box[2 * g], h = (double)box[2 * g + 1];
                const LocBox d{x, x + w, y, y + h};
                const double a_gt = w * h;
                for (int t = 0; t < ninf; ++t) {
                    if ((used_t >> t) & 1u) continue;
                    const LocPair p = loc_pair(loc_inferred_box(rec0 + t * rec_step, q, C), d, a_gt);
                    if (p.iou > best) { best = p.iou; bg = g; bt = t; }
                }
            }
            if (bg < 0) break;
            used_g |= 1u << bg;
            used_t |= 1u << bt;
            steps |= (uint64_t)bt << (4 * bg);
        }
        int hits = 0;
        for (int g = 0; g < G; ++g) {
            const bool taken = (used_g >> g) & 1u;               // (only digits below cnt are ever used)
            const int t = (int)((steps >> (4 * g)) & 15u);
            double v = 0.0;
            if (taken) {
                const int32_t px = pos[2 * g], py = pos[2 * g + 1], bw = box[2 * g], bh = box[2 * g + 1];
                const double x = (double)px, y = (double)py, w = (double)bw, h = (double)bh;
                const LocBox d{x, x + w, y, y + h};
                const float* rec = rec0 + t * rec_step;
                const LocPair p = loc_pair(loc_inferred_box(rec, q, C), d, w * h);
                const double cx = ((double)(px + px + bw) - 1.0) / 2.0, cy = ((double)(py + py + bh) - 1.0) / 2.0;
                const double x1 = cx / half - 1.0, y1 = cy / half - 1.0;
                const double dx = (double)rec[AIR_ATT_X] - x1, dy = (double)rec[AIR_ATT_Y] - y1;
                v = p.iou;
                s_iou = s_iou + p.iou;
                s_cover = s_cover + p.cover;
                s_dist = s_dist + sqrt(dx * dx + dy * dy);
                hits += p.iou >= a.iou_threshold ? 1 : 0;
            }
            if (a.match) {
                a.match[(int64_t)i * G + g] = taken ? t : -1;
                a.iou[(int64_t)i * G + g] = v;
            }
        }
        const int matched = __popc(used_g);
        atomicAdd(&tally[AIR_LOC_IMAGES], 1);                    // integer LDS atomics: any order, the same sums
        if (cnt) atomicAdd(&tally[AIR_LOC_PRESENT], cnt);
        if (ninf) atomicAdd(&tally[AIR_LOC_INFERRED], ninf);
        if (matched) atomicAdd(&tally[AIR_LOC_MATCHED], matched);
        if (hits) atomicAdd(&tally[AIR_LOC_HITS], hits);
        if (cnt == ninf) atomicAdd(&tally[AIR_LOC_COUNT_CORRECT], 1);
        atomicAdd(&tally[AIR_LOC_COUNTS + cnt * (T + 1) + ninf], 1);
    }
    const double g_iou = loc_group_tree(s_iou, red[AIR_LOC_IOU]);
    const double g_cover = loc_group_tree(s_cover, red[AIR_LOC_COVER]);
    const double g_dist = loc_group_tree(s_dist, red[AIR_LOC_DIST]);     // (its barrier also closes the tally)
    if (tid == 0) {
        double* out = partials + (int64_t)blockIdx.x * AIR_LOC_SUMS;
        out[AIR_LOC_IOU] = g_iou; out[AIR_LOC_COVER] = g_cover; out[AIR_LOC_DIST] = g_dist;
    }
    for (int j = tid; j < ncounts; j += LOC_THREADS) {
        const int32_t v = tally[j];
        if (v) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + j, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(64) void loc_fold_kernel(const double* __restrict__ partials, int groups, double* __restrict__ sums) {
    const int j = threadIdx.x;
    if (j >= AIR_LOC_SUMS) return;
    double total = 0.0;
    for (int g = 0; g < groups; ++g) total = total + partials[(int64_t)g * AIR_LOC_SUMS + j];
    sums[j] = sums[j] + total;
}

int loc_check(int T, int B, int k, int G) {
    if (T < 1 || B < 1 || k < 1 || G < 1 || k > B) return AIR_EINVAL;
    if (T > AIR_LOC_MAX_STEPS || G > AIR_LOC_MAX_DIGITS) return AIR_ELIMIT;
    return 0;
}

int loc_groups(int k) { return (int)(((int64_t)k + LOC_THREADS - 1) / LOC_THREADS); }

}  // namespace

extern "C" int64_t air_localization_workspace_bytes(int T, int B, int k, int G) {
    const int rc = loc_check(T, B, k, G);
    return rc ? rc : (int64_t)loc_groups(k) * AIR_LOC_SUMS * (int64_t)sizeof(double);
}

extern "C" int air_localization(const air_localization_t* a, void* workspace, void* stream) {
    if (!a) return AIR_EINVAL;
    const int rc = loc_check(a->T, a->B, a->k, a->G);
    if (rc) return rc;
    if (a->canvas_size < 2 || !(a->iou_threshold > 0.0 && a->iou_threshold <= 1.0)) return AIR_EINVAL;
    if (!a->att || !a->run_digits || !a->gt_count || !a->gt_positions || !a->gt_boxes || !a->counts || !a->sums || !workspace)
        return AIR_EINVAL;
    if (!a->match != !a->iou) return AIR_EINVAL;
    hipStream_t s = air_stream(stream);
    const int groups = loc_groups(a->k);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(loc_match_kernel, dim3(groups), dim3(LOC_THREADS), 0, s, *a, partials);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(loc_fold_kernel, dim3(1), dim3(64), 0, s, partials, groups, a->sums);
    AIR_CHECK_LAUNCH();
    return 0;
}
