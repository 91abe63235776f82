// Handwriting bank: base glyphs distorted into MNIST's geometry on the device, one workgroup per variant -- see
// air_glyph_distort_t in air_hip.h for the semantics, the draw order, every operation of the six stages and the status values.
//
// Stages: elastic field (two planes of uniform draws, smoothed along axis 0 then axis 1, times field_gain) -> warp (affine +
// field, bilinear read of the base plane, float32) -> stroke (|n| passes of grey dilation / erosion over the 4-neighbour cross)
// -> ramp (clip, threshold, box) -> fit (area average onto ink pixels a side, threshold, box) -> centre (centre of mass onto
// the middle of the od x od frame).  The build has -ffp-contract=off and every operation but cos / sin of the angle is an
// IEEE +, -, *, /, floor, min or max in fp64, so tests/glyph_distort_cases.py restates the kernel bit for bit.
//
// Control flow is uniform: the parameter draws are computed by every thread from blockIdx and uniform arguments, and
// everything data-dependent (a box, hence the status) is read from LDS behind a barrier by all threads -- every branch that
// holds a barrier is reached by all threads of the workgroup or by none.  Trip counts: a plane has gd * gd <= 40 * 40 pixels,
// a tap line 2 * radius + 1 <= 129 taps, a stroke |n| <= 4 passes, a fitted plane at most od x gd <= 32 x 40 pixels, all
// range-checked by distort_check before the launch.  No global atomics; the boxes are LDS min / max.
//
// LDS (all dynamic, distort_lds() is the one place that sizes it), with S = max(gd, od):
//   fa, fb, fc [S * S] double each | taps [2 * radius + 1] double | base [S * S] float | meta [8] int.
//   fa / fc: the uniform planes, then the field (axis 0 goes through fb).  After the warp: fb and fa as float planes are the
//   two sides of the stroke passes, then the row sums of the centre of mass; fc holds the fit's axis-0 result; base holds the
//   base glyph, then the fitted glyph.  meta: the box (min x, min y, max x, max y) of the ramp, then of the fit.
//   45 864 bytes at the limits (S = 40, radius = 64): below 48 KiB, so no grant is needed.
#include <cmath>

#include "air_common.h"
#include "air_philox.h"

namespace {

constexpr int GD_THREADS = 256;
constexpr uint32_t GD_SALT_P = 0x47445350u;       // the parameter stream
constexpr uint32_t GD_SALT_F = 0x47445346u;       // the field stream
constexpr int GD_META_INTS = 8;

struct DistortLds { size_t fa, fb, fc, taps, base, meta, total; };      // byte offsets of the parts, and the request
inline DistortLds distort_lds(int gd, int od, int radius) {
    const size_t S = (size_t)(gd > od ? gd : od), plane = sizeof(double) * S * S;
    DistortLds L;
    L.fa = 0;
    L.fb = plane;
    L.fc = 2 * plane;
    L.taps = 3 * plane;
    L.base = L.taps + sizeof(double) * (2 * (size_t)radius + 1);
    L.meta = L.base + sizeof(float) * S * S;
    L.total = L.meta + sizeof(int) * GD_META_INTS;
    return L;
}

// one pass of the smoothing: dst[y, x] = sum over t = first .. last tap, ascending, of taps[t] * src at offset t - R along the
// axis; the taps whose pixel lies outside the plane are left out (they would add +0).  `gain` multiplies the sum.
__device__ __forceinline__ void gd_smooth(const double* src, double* dst, const double* taps, int gd, int R, int axis, double gain) {
    for (int p = threadIdx.x; p < gd * gd; p += GD_THREADS) {
        const int y = p / gd, x = p - y * gd;
        const int at = axis == 0 ? y : x, step = axis == 0 ? gd : 1;
        const int t0 = R - at > 0 ? R - at : 0, t1 = R + gd - 1 - at < 2 * R ? R + gd - 1 - at : 2 * R;
        const double* line = src + p + (t0 - R) * step;
        double acc = 0.0;
        for (int t = t0; t <= t1; ++t) {
            acc = acc + taps[t] * *line;
            line += step;
        }
        dst[p] = acc * gain;
    }
}

// the length of the overlap of output cell i = [lo, hi) with input cell j = [j, j + 1)
__device__ __forceinline__ double gd_overlap(double lo, double hi, int j) {
    const double ov = fmin((double)(j + 1), hi) - fmax((double)j, lo);
    return ov > 0.0 ? ov : 0.0;
}

__device__ __forceinline__ void gd_box(int* box, int x0, int y0, int x1, int y1) {
    if (x1 >= 0) {                                                    // (LDS atomics; no thread waits on another's)
        atomicMin(&box[0], x0); atomicMin(&box[1], y0);
        atomicMax(&box[2], x1); atomicMax(&box[3], y1);
    }
}

__global__ __launch_bounds__(GD_THREADS) void glyph_distort_kernel(air_glyph_distort_t a, DistortLds L) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gd_lds[];
    double* fa = reinterpret_cast<double*>(gd_lds + L.fa);
    double* fb = reinterpret_cast<double*>(gd_lds + L.fb);
    double* fc = reinterpret_cast<double*>(gd_lds + L.fc);
    double* taps = reinterpret_cast<double*>(gd_lds + L.taps);
    float* base = reinterpret_cast<float*>(gd_lds + L.base);
    int* meta = reinterpret_cast<int*>(gd_lds + L.meta);
    const int tid = threadIdx.x, v = blockIdx.x, gd = a.gd, od = a.od, N = gd * gd, R = a.radius;
    const uint32_t generation = (uint32_t)(a.counter ? *a.counter : (int64_t)0);

    // the parameter draws of one variant (at most 10 words: three quads)
    AirDraws<GD_SALT_P> d((uint32_t)v, generation, a.seed);
    const int g = d.range(0, a.G);
    double ang = 0.0, k = 0.0, sx = 1.0, sy = 1.0, c = 1.0, s = 0.0;
    int n = 0;
    if (a.max_ang != 0.0) {
        ang = d.real(-a.max_ang, a.max_ang);
        // |ang| <= 180: q = the nearest multiple of 90, r = ang - 90 q exactly, |r| <= 45; cos, sin of r by sincospi
        const double q = rint(ang / 90.0), r = ang - 90.0 * q;
        double sr, cr;
        sincospi(r / 180.0, &sr, &cr);
        const int qi = (int)q & 3;
        c = qi == 0 ? cr : qi == 1 ? -sr : qi == 2 ? -cr : sr;
        s = qi == 0 ? sr : qi == 1 ? cr : qi == 2 ? -sr : -cr;
    }
    if (a.max_shear != 0.0) k = d.real(-a.max_shear, a.max_shear);
    if (a.min_scale != 1.0 || a.max_scale != 1.0) {
        sx = d.real(a.min_scale, a.max_scale);
        sy = d.real(a.min_scale, a.max_scale);
    }
    if (a.min_stroke != 0 || a.max_stroke != 0) n = d.range(a.min_stroke, a.max_stroke - a.min_stroke + 1);
    const bool field = a.field_gain != 0.0;

    if (tid < GD_META_INTS) meta[tid] = (tid & 3) < 2 ? INT_MAX : -1;
    const float* src = a.glyphs + (size_t)g * N;
    for (int p = tid; p < N; p += GD_THREADS) base[p] = src[p];
    for (int t = tid; t < 2 * R + 1; t += GD_THREADS) taps[t] = a.taps[t];

    // 1. the elastic field: element j = plane * N + y * gd + x is word j & 3 of quad j >> 2 of the field stream
    if (field) {
        const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
        for (int q = tid; q < (2 * N + 3) / 4; q += GD_THREADS) {
            uint32_t w[4] = {(uint32_t)v, (uint32_t)q, generation, GD_SALT_F};
            air_philox4x32_10(w, k0, k1);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int j = 4 * q + e;
                const double u = ((double)(w[e] >> 8) + 0.5) * 1.1920928955078125e-7 - 1.0;
                if (j < N) fa[j] = u;
                else if (j < 2 * N) fc[j - N] = u;
            }
        }
        __syncthreads();
        gd_smooth(fa, fb, taps, gd, R, 0, 1.0);
        __syncthreads();
        gd_smooth(fb, fa, taps, gd, R, 1, a.field_gain);
        __syncthreads();
        gd_smooth(fc, fb, taps, gd, R, 0, 1.0);
        __syncthreads();
        gd_smooth(fb, fc, taps, gd, R, 1, a.field_gain);
    }
    __syncthreads();

    // 2. the warp: fb as a float plane, row stride gd
    float* cur = reinterpret_cast<float*>(fb);
    float* other = reinterpret_cast<float*>(fa);
    {
        const double isy = 1.0 / sy, isx = 1.0 / sx, ctr = ((double)gd - 1.0) / 2.0;
        const double a00 = c * isy, a01 = (c * k + s) * isx, a10 = (-s) * isy, a11 = ((-s) * k + c) * isx;
        for (int p = tid; p < N; p += GD_THREADS) {
            const int y = p / gd, x = p - y * gd;
            const double dy = (double)y - ctr, dx = (double)x - ctr;
            double qy = ctr + (a00 * dy + a01 * dx), qx = ctr + (a10 * dy + a11 * dx);
            if (field) { qy = qy + fa[p]; qx = qx + fc[p]; }
            float r = 0.0f;
            if (qy > -1.0 && qy < (double)gd && qx > -1.0 && qx < (double)gd) {       // (else all four pixels are outside)
                const double fy = floor(qy), fx = floor(qx), ty = qy - fy, tx = qx - fx;
                const int iy = (int)fy, ix = (int)fx;
                const bool y0 = iy >= 0, y1 = iy + 1 < gd, x0 = ix >= 0, x1 = ix + 1 < gd;
                const double v00 = y0 && x0 ? (double)base[iy * gd + ix] : 0.0;
                const double v01 = y0 && x1 ? (double)base[iy * gd + ix + 1] : 0.0;
                const double v10 = y1 && x0 ? (double)base[(iy + 1) * gd + ix] : 0.0;
                const double v11 = y1 && x1 ? (double)base[(iy + 1) * gd + ix + 1] : 0.0;
                const double uy = 1.0 - ty, ux = 1.0 - tx;
                r = (float)(((v00 * (uy * ux) + v01 * (uy * tx)) + v10 * (ty * ux)) + v11 * (ty * tx));
            }
            cur[p] = r;
        }
    }
    __syncthreads();                                                  // (also: every read of the field and the base is done)

    // 3. the stroke: |n| passes over the cross (centre, up, down, left, right), the neighbours outside the plane left out
    for (int pass = 0; pass < (n < 0 ? -n : n); ++pass) {
        for (int p = tid; p < N; p += GD_THREADS) {
            const int y = p / gd, x = p - y * gd;
            float m = cur[p];
            if (n > 0) {
                if (y > 0) m = fmaxf(m, cur[p - gd]);
                if (y + 1 < gd) m = fmaxf(m, cur[p + gd]);
                if (x > 0) m = fmaxf(m, cur[p - 1]);
                if (x + 1 < gd) m = fmaxf(m, cur[p + 1]);
            } else {
                if (y > 0) m = fminf(m, cur[p - gd]);
                if (y + 1 < gd) m = fminf(m, cur[p + gd]);
                if (x > 0) m = fminf(m, cur[p - 1]);
                if (x + 1 < gd) m = fminf(m, cur[p + 1]);
            }
            other[p] = m;
        }
        __syncthreads();
        float* t = cur; cur = other; other = t;
    }

    // 4. the ramp, in place, and its box
    {
        const double span = a.hi - a.lo;
        int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
        for (int p = tid; p < N; p += GD_THREADS) {
            const int y = p / gd, x = p - y * gd;
            double t = ((double)cur[p] - a.lo) / span;
            t = t < 0.0 ? 0.0 : t > 1.0 ? 1.0 : t;
            float r = (float)t;
            if (r < 0.05f) r = 0.0f;
            cur[p] = r;
            if (r > 0.0f) {
                x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
                y0 = y < y0 ? y : y0; y1 = y > y1 ? y : y1;
            }
        }
        gd_box(meta, x0, y0, x1, y1);
    }
    __syncthreads();
    int status = meta[2] < 0 ? 1 : 0;
    int bx = 0, by = 0, bw = 0, bh = 0, ps = 0;
    double f = 0.0, cy = 0.0, cx = 0.0;

    // 5. the fit: the box (h x w) of `cur` onto h2 x w2, the larger side ink; the result in `base`, row stride w2
    if (status == 0) {
        const int ix = meta[0], iy = meta[1], w = meta[2] - ix + 1, h = meta[3] - iy + 1;
        f = (double)a.ink / (double)(h > w ? h : w);
        const double fh = floor((double)h * f + 0.5), fw = floor((double)w * f + 0.5);
        const int h2 = fh < 1.0 ? 1 : (int)fh, w2 = fw < 1.0 ? 1 : (int)fw;          // (<= ink <= od: h f, w f <= ink (1 + 2^-52))
        const double rh = (double)h / (double)h2, rw = (double)w / (double)w2;
        ps = w2;
        for (int p = tid; p < h2 * w; p += GD_THREADS) {
            const int i = p / w, x = p - i * w;
            const double lo = (double)i * rh, hi = (double)(i + 1) * rh;
            double acc = 0.0;
            for (int j = 0; j < h; ++j) acc = acc + (double)cur[(iy + j) * gd + ix + x] * gd_overlap(lo, hi, j);
            fc[p] = acc / rh;
        }
        __syncthreads();
        int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
        for (int p = tid; p < h2 * w2; p += GD_THREADS) {
            const int i = p / w2, x = p - i * w2;
            const double lo = (double)x * rw, hi = (double)(x + 1) * rw;
            double acc = 0.0;
            for (int j = 0; j < w; ++j) acc = acc + fc[i * w + j] * gd_overlap(lo, hi, j);
            float r = (float)(acc / rw);
            if (r < 0.05f) r = 0.0f;
            base[p] = r;
            if (r > 0.0f) {
                x0 = x < x0 ? x : x0; x1 = x > x1 ? x : x1;
                y0 = i < y0 ? i : y0; y1 = i > y1 ? i : y1;
            }
        }
        gd_box(meta + 4, x0, y0, x1, y1);
        __syncthreads();                                              // (also: every read of cur is done: fa, fb are free)
        if (meta[6] < 0) status = 1;
        else {
            bx = meta[4]; by = meta[5]; bw = meta[6] - bx + 1; bh = meta[7] - by + 1;
            // 6. the centre of mass of the box: per row the sums of v and of v * x, x ascending; then the rows, ascending
            if (tid < bh) {
                double m = 0.0, mx = 0.0;
                for (int x = 0; x < bw; ++x) {
                    const double val = (double)base[(by + tid) * w2 + bx + x];
                    m = m + val;
                    mx = mx + val * (double)x;
                }
                fa[tid] = m;
                fb[tid] = mx;
            }
            __syncthreads();
            double m = 0.0, my = 0.0, mx = 0.0;
            for (int r = 0; r < bh; ++r) {
                m = m + fa[r];
                my = my + fa[r] * (double)r;
                mx = mx + fb[r];
            }
            cy = my / m;
            cx = mx / m;
            if (bw > od || bh > od) status = 2;                       // (ink <= od rules it out; nothing is written outside)
        }
    }
    int px0 = 0, py0 = 0;
    if (status == 0) {
        const double mid = ((double)od - 1.0) / 2.0;
        double ty = floor(mid - cy + 0.5), tx = floor(mid - cx + 0.5);
        const double my = (double)(od - bh), mx = (double)(od - bw);
        ty = ty < 0.0 ? 0.0 : ty > my ? my : ty;
        tx = tx < 0.0 ? 0.0 : tx > mx ? mx : tx;
        py0 = (int)ty;
        px0 = (int)tx;
    }

    float* out = a.bank + (size_t)v * od * od;
    for (int p = tid; p < od * od; p += GD_THREADS) {
        const int y = p / od - py0, x = p % od - px0;
        out[p] = status == 0 && y >= 0 && y < bh && x >= 0 && x < bw ? base[(by + y) * ps + bx + x] : 0.0f;
    }
    if (tid == 0) {
        *reinterpret_cast<int4*>(a.bank_crops + (size_t)v * 4) = status == 0 ? make_int4(px0, py0, bw, bh) : make_int4(0, 0, 0, 0);
        a.source[v] = g;
        a.status[v] = status;
    }
    if (tid < 8)
        a.params[(size_t)v * 8 + tid] = tid == 0 ? ang : tid == 1 ? k : tid == 2 ? sx : tid == 3 ? sy : tid == 4 ? c : tid == 5 ? s :
                                        tid == 6 ? (double)n : f;
}

int distort_check_sizes(int gd, int od, int radius) {
    if (gd < 1 || od < 1 || radius < 0) return AIR_EINVAL;
    if (gd > AIR_DISTORT_MAX_PLANE || od > AIR_SCENE_MAX_GLYPH || radius > AIR_DISTORT_MAX_RADIUS) return AIR_ELIMIT;
    return 0;
}

// an invalid size before a limit, a limit before a null pointer, a null pointer before the alignment
int distort_check(const air_glyph_distort_t* a) {
    if (!a) return AIR_EINVAL;
    if (a->V < 1 || a->G < 1 || a->gd < 1 || a->od < 1 || a->ink < 1 || a->radius < 0 || a->ink > a->od) return AIR_EINVAL;
    const double b[7] = {a->field_gain, a->max_ang, a->max_shear, a->min_scale, a->max_scale, a->lo, a->hi};
    for (double x : b) if (!std::isfinite(x)) return AIR_EINVAL;
    if (a->min_scale > a->max_scale || a->min_stroke > a->max_stroke || !(a->lo < a->hi)) return AIR_EINVAL;
    if (a->min_scale <= 0.0) return AIR_EINVAL;
    if (int rc = distort_check_sizes(a->gd, a->od, a->radius)) return rc;
    if (std::fabs(a->max_ang) > 180.0) return AIR_ELIMIT;
    if (a->min_stroke < -AIR_DISTORT_MAX_STROKE || a->max_stroke > AIR_DISTORT_MAX_STROKE) return AIR_ELIMIT;
    if (!a->glyphs || !a->taps || !a->bank || !a->bank_crops || !a->source || !a->params || !a->status) return AIR_EINVAL;
    if ((uintptr_t)a->bank_crops & 15) return AIR_EALIGN;                     // a crop box is one 16-byte store
    if (((uintptr_t)a->params & 7) || ((uintptr_t)a->taps & 7)) return AIR_EALIGN;
    return 0;
}

}  // namespace

extern "C" int64_t air_glyph_distort_lds(int gd, int od, int radius) {
    if (int rc = distort_check_sizes(gd, od, radius)) return rc;
    return (int64_t)distort_lds(gd, od, radius).total;
}

extern "C" int air_glyph_distort_prepare(const air_glyph_distort_t* a) {
    if (int rc = distort_check(a)) return rc;
    return air_grant_lds(reinterpret_cast<const void*>(&glyph_distort_kernel), distort_lds(a->gd, a->od, a->radius).total);
}

extern "C" int air_glyph_distort(const air_glyph_distort_t* a, void* stream) {
    if (int rc = distort_check(a)) return rc;
    const DistortLds L = distort_lds(a->gd, a->od, a->radius);
    if (int rc = air_grant_lds(reinterpret_cast<const void*>(&glyph_distort_kernel), L.total)) return rc;
    hipLaunchKernelGGL(glyph_distort_kernel, dim3(a->V), dim3(GD_THREADS), L.total, air_stream(stream), *a, L);
    AIR_CHECK_LAUNCH();
    return 0;
}
