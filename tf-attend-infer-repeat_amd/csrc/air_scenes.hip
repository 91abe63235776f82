// Scene source: the default path of the reference's generate_multi_image (multi_mnist.py:82-183, use_pixel_overlap=True,
// no jitter) composed on the device, one workgroup per scene -- see air_scene_source_t in air_hip.h for the semantics, the
// draw order and the two deviations from the reference.
//
// Everything a scene decides is decided by EVERY thread of its workgroup from the same integers: the Philox draws are
// computed redundantly per thread (they depend on blockIdx and on uniform counters only), and the one data-dependent
// answer, "does this placement touch ink", is a workgroup-wide OR read by all threads behind a barrier -- so every branch and every barrier
// below is reached by all threads or by none.  Trip counts: restarts < max_restarts <= 64, digits < n <= max_digits <= 6,
// attempts < max_attempts <= 100, all range-checked by scene_check before the launch.
//
// LDS (all dynamic, every part 16-byte aligned; scene_lds() is the one place that sizes it):
//   canvas [C * C] float | glyph [gd * gd] float, the crop box of the glyph being placed, row stride w | occupancy [C * C]
//   bytes, 1 = within Chebyshev distance `gap` of ink on the canvas | meta [40] int: indices 0..5, positions 6..17, boxes
//   18..29, the OR's flag words 32..34.  No static LDS: the dynamic part may then be granted up to the whole 160 KiB.
#include "air_common.h"
#include "air_philox.h"

namespace {

constexpr int SC_THREADS = 256;
constexpr uint32_t SC_SALT = 0x5343454Eu;
constexpr int SC_META_INTS = 40;
constexpr int SC_FLAGS = 32;          // meta[32..34]: the flag words of the workgroup-wide OR

struct SceneLds { size_t canvas, glyph, occ, meta, total; };      // byte offsets of the parts, and the request
inline SceneLds scene_lds(int C, int gd) {
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    SceneLds L;
    L.canvas = 0;
    L.glyph = up16(sizeof(float) * (size_t)C * C);
    L.occ = L.glyph + up16(sizeof(float) * (size_t)gd * gd);
    L.meta = L.occ + up16((size_t)C * C);
    L.total = L.meta + sizeof(int) * SC_META_INTS;
    return L;
}

__global__ __launch_bounds__(SC_THREADS) void scene_compose_kernel(air_scene_source_t a, int step_in_replay, size_t off_glyph,
                                                                   size_t off_occ, size_t off_meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sc_lds[];
    float* canvas = reinterpret_cast<float*>(sc_lds);
    float* glyph = reinterpret_cast<float*>(sc_lds + off_glyph);
    unsigned char* occ = sc_lds + off_occ;
    int* meta = reinterpret_cast<int*>(sc_lds + off_meta);
    const int tid = threadIdx.x, b = blockIdx.x;
    const int C = a.C, CC = C * C, gd = a.gd, gap = a.gap, margin = a.margin;
    const int n16_canvas = (int)(off_glyph / 16), n16_occ = (int)((off_meta - off_occ) / 16);

    AirDraws<SC_SALT> d((uint32_t)b, (uint32_t)(*a.batch_counter + (int64_t)step_in_replay), a.seed);    // the draws of one scene

    int n;
    if (a.counts) {
        n = a.counts[b];
        n = n < 0 ? 0 : (n > a.max_digits ? a.max_digits : n);
    } else
        n = d.range(0, a.max_digits + 1);

    bool ok = false;
    int restarts = 0, tests = 0;      // tests: overlap tests made so far (picks the flag word of the next one)
    for (; restarts < a.max_restarts; ++restarts) {
        // both planes to zero, in 16-byte stores over their rounded-up parts (+0.0f is all-zero bits)
        for (int i = tid; i < n16_canvas; i += SC_THREADS) reinterpret_cast<uint4*>(sc_lds)[i] = make_uint4(0, 0, 0, 0);
        for (int i = tid; i < n16_occ; i += SC_THREADS) reinterpret_cast<uint4*>(occ)[i] = make_uint4(0, 0, 0, 0);
        if (tid < SC_META_INTS) meta[tid] = 0;
        ok = true;
        for (int i = 0; i < n; ++i) {
            const int g = d.range(0, a.G);
            const int4 box = *reinterpret_cast<const int4*>(a.crops + (size_t)g * 4);
            const int x0 = box.x, y0 = box.y, w = box.z, h = box.w;
            const bool box_ok = w >= 1 && h >= 1 && x0 >= 0 && y0 >= 0 && x0 + w <= gd && y0 + h <= gd;
            if (!box_ok || w + 2 * margin > C || h + 2 * margin > C) { ok = false; break; }
            const int hw = h * w;
            const float* src = a.glyphs + (size_t)g * gd * gd;
            for (int p = tid; p < hw; p += SC_THREADS) {
                const int py = p / w, px = p - py * w;
                glyph[p] = src[(y0 + py) * gd + x0 + px];
            }
            __syncthreads();          // the glyph is staged; the canvas / occupancy of the scene so far is complete
            bool found = false;
            int x = 0, y = 0;
            for (int t = 0; t < a.max_attempts; ++t) {
                x = d.range(margin, C - w - 2 * margin + 1);          // [margin, C - w - margin]
                y = d.range(margin, C - h - 2 * margin + 1);
                if (i == 0) { found = true; break; }
                int hit = 0;
                for (int p = tid; p < hw; p += SC_THREADS) {
                    const int py = p / w, px = p - py * w;
                    hit |= (glyph[p] > 0.0f) & (occ[(y + py) * C + x + px] != 0);
                }
                // workgroup-wide OR through one of three flag words in turn, one barrier per test: test k sets flag k % 3
                // and clears flag (k + 1) % 3, which was last read behind the barrier of test k - 2 -- every thread has
                // passed the barrier of test k - 1 since.  (All LDS is dynamic: __syncthreads_or brings a static block, and
                // the 160 KiB grant is for the dynamic part alone.)
                const int slot = SC_FLAGS + tests % 3, next = SC_FLAGS + (tests + 1) % 3;
                ++tests;
                if (tid == 0) meta[next] = 0;
                if (__any(hit) && (tid & 63) == 0) meta[slot] = 1;
                __syncthreads();
                found = meta[slot] == 0;
                if (found) break;
            }
            if (!found) { ok = false; break; }
            for (int p = tid; p < hw; p += SC_THREADS) {
                const int py = p / w, px = p - py * w;
                const float v = glyph[p];
                const int cy = y + py, cx = x + px;
                canvas[cy * C + cx] += v;                                   // (this thread alone owns the pixel)
                if (v > 0.0f) {
                    const int ya = cy - gap < 0 ? 0 : cy - gap, yb = cy + gap >= C ? C - 1 : cy + gap;
                    const int xa = cx - gap < 0 ? 0 : cx - gap, xb = cx + gap >= C ? C - 1 : cx + gap;
                    for (int yy = ya; yy <= yb; ++yy)
                        for (int xx = xa; xx <= xb; ++xx) occ[yy * C + xx] = 1;   // (several threads may store the same 1)
                }
            }
            if (tid == 0) {
                meta[i] = g;
                meta[6 + 2 * i] = x; meta[7 + 2 * i] = y;
                meta[18 + 2 * i] = w; meta[19 + 2 * i] = h;
            }
            __syncthreads();          // pasted: the glyph buffer may be restaged, the planes read
        }
        __syncthreads();              // (a failed scene: every read of its planes before they are cleared)
        if (ok) break;
    }
    if (!ok) {                        // gave up: an empty canvas
        for (int i = tid; i < CC; i += SC_THREADS) canvas[i] = 0.0f;
        if (tid < SC_META_INTS) meta[tid] = 0;
        __syncthreads();
    }

    float* out = a.images + (size_t)b * CC;
    const bool vec = (CC & 3) == 0 && ((uintptr_t)a.images & 15) == 0 && (!a.bg || ((uintptr_t)a.bg & 15) == 0);
    if (vec) {
        for (int i = tid; i < CC / 4; i += SC_THREADS) {
            float4 v = reinterpret_cast<const float4*>(canvas)[i];
            if (a.bg) {
                const float4 g = reinterpret_cast<const float4*>(a.bg)[i];
                v.x = fminf(fmaxf(v.x + g.x, 0.0f), 1.0f); v.y = fminf(fmaxf(v.y + g.y, 0.0f), 1.0f);
                v.z = fminf(fmaxf(v.z + g.z, 0.0f), 1.0f); v.w = fminf(fmaxf(v.w + g.w, 0.0f), 1.0f);
            }
            reinterpret_cast<float4*>(out)[i] = v;
        }
    } else {
        for (int i = tid; i < CC; i += SC_THREADS) {
            float v = canvas[i];
            if (a.bg) v = fminf(fmaxf(v + a.bg[i], 0.0f), 1.0f);
            out[i] = v;
        }
    }
    const int md = a.max_digits;
    if (tid < md) a.indices[(size_t)b * md + tid] = meta[tid];
    if (tid < 2 * md) {
        a.positions[(size_t)b * 2 * md + tid] = meta[6 + tid];
        a.boxes[(size_t)b * 2 * md + tid] = meta[18 + tid];
    }
    if (tid == 0) {
        a.digits[b] = ok ? n : 0;
        a.status[b] = ok ? restarts : -1;
        if (a.gave_up) a.gave_up[b] += ok ? 0 : 1;
    }
}

__global__ void scene_advance_kernel(int64_t* counter, int by) { *counter += by; }

// an invalid size before a limit, a limit before a null pointer
int scene_check_sizes(int C, int gd) {
    if (C < 1 || gd < 1) return AIR_EINVAL;
    if (C > AIR_SCENE_MAX_CANVAS || gd > AIR_SCENE_MAX_GLYPH) return AIR_ELIMIT;
    return 0;
}

int scene_check(const air_scene_source_t* a, int step_in_replay) {
    if (!a) return AIR_EINVAL;
    if (a->B < 1 || a->G < 1 || a->gd < 1 || a->C < 1 || a->max_digits < 1 || a->margin < 0 || a->gap < 0 ||
        step_in_replay < 0 || a->max_attempts < 1 || a->max_restarts < 1) return AIR_EINVAL;
    if (2 * (int64_t)a->margin + 1 > a->C) return AIR_EINVAL;                 // not even a one-pixel glyph fits
    if (int rc = scene_check_sizes(a->C, a->gd)) return rc;
    if (a->max_digits > AIR_SCENE_MAX_DIGITS || a->gap > AIR_SCENE_MAX_GAP || a->max_attempts > AIR_SCENE_MAX_ATTEMPTS ||
        a->max_restarts > AIR_SCENE_MAX_RESTARTS) return AIR_ELIMIT;
    if (!a->glyphs || !a->crops || !a->batch_counter || !a->images || !a->digits || !a->indices || !a->positions ||
        !a->boxes || !a->status) return AIR_EINVAL;
    if ((uintptr_t)a->crops & 15) return AIR_EALIGN;                          // a crop box is one 16-byte load
    return 0;
}

int scene_grant(const air_scene_source_t* a, SceneLds* L) {
    *L = scene_lds(a->C, a->gd);
    return air_grant_lds(reinterpret_cast<const void*>(&scene_compose_kernel), L->total);
}

}  // namespace

extern "C" int64_t air_scene_source_lds(int C, int gd) {
    if (int rc = scene_check_sizes(C, gd)) return rc;
    return (int64_t)scene_lds(C, gd).total;
}

extern "C" int air_scene_source_prepare(const air_scene_source_t* a) {
    if (int rc = scene_check(a, 0)) return rc;
    SceneLds L;
    return scene_grant(a, &L);
}

extern "C" int air_scene_source_compose(const air_scene_source_t* a, int step_in_replay, void* stream) {
    if (int rc = scene_check(a, step_in_replay)) return rc;
    SceneLds L;
    if (int rc = scene_grant(a, &L)) return rc;
    hipLaunchKernelGGL(scene_compose_kernel, dim3(a->B), dim3(SC_THREADS), L.total, air_stream(stream), *a, step_in_replay,
                       L.glyph, L.occ, L.meta);
    AIR_CHECK_LAUNCH();
    return 0;
}

extern "C" int air_scene_source_advance(int64_t* counter, int by, void* stream) {
    if (!counter || by < 0) return AIR_EINVAL;
    hipLaunchKernelGGL(scene_advance_kernel, dim3(1), dim3(1), 0, air_stream(stream), counter, by);
    AIR_CHECK_LAUNCH();
    return 0;
}
