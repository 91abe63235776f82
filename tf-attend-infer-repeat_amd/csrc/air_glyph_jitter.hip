// Glyph bank: the scale and rotation jitter of the reference's generate_multi_image (multi_mnist.py:113-135) on the device,
// one workgroup per variant -- see air_glyph_jitter_t in air_hip.h for the semantics, the draw order and the status values.
//
// Both stages are scipy's affine_transform(order=5, mode='constant', cval=0, prefilter=True) in fp64: the order-5 B-spline
// prefilter (mirror boundaries; axis 0, then axis 1; one line per thread, a barrier between the axes), then one output pixel
// per thread at a time -- 6 x 6 taps, the products (coefficient * wy) * wx summed row by row from the top-left tap --
// rounded to float32, clipped to [0, 1], values < 0.05 zeroed, and the box of what is left found by LDS min / max.  The build
// has -ffp-contract=off and every operation but cos / sin of the angle is an IEEE +, -, *, / or floor, so
// tests/glyph_jitter_cases.py restates the kernel bit for bit.  The two poles and the gain come from the host (its sqrt is
// correctly rounded) as kernel arguments.
//
// Control flow is uniform: the draws are computed by every thread from blockIdx and uniform arguments, and everything
// data-dependent (a stage's box, hence the status) is read from LDS behind a barrier by all threads -- every branch and
// barrier below is reached by all threads of the workgroup or by none.  Trip counts: a line has at most GJ_ROT = 64
// elements, a plane at most 64 x 64 pixels, both checked in the kernel before the plane is touched; gd, od <= 32 and the
// scaled plane <= 48 a side are range-checked by jitter_check before the launch.
//
// LDS (all dynamic, jitter_lds() is the one place that sizes it; the same at every (gd, od), sized for the limits):
//   coef [48 * 48] double, the coefficients of the stage's input | plane [64 * 64] float, the image so far: the base crop,
//   then each stage's output | meta [8] int: the box (min x, min y, max x, max y) of the scale stage, then of the rotation.
#include <cmath>

#include "air_common.h"
#include "air_philox.h"

namespace {

constexpr int GJ_THREADS = 256;
constexpr uint32_t GJ_SALT = 0x474A4954u;
constexpr int GJ_ROT = 64;            // the largest rotated plane, a side (a 48 x 48 input at 45 degrees would need 68)
constexpr int GJ_META_INTS = 8;

struct JitterLds { size_t coef, plane, meta, total; };            // byte offsets of the parts, and the request
inline JitterLds jitter_lds(int /*gd*/, int /*od*/) {             // gd <= 32 < 48 and od <= 32 < 64: the limits size it
    JitterLds L;
    L.coef = 0;
    L.plane = sizeof(double) * AIR_JITTER_MAX_PLANE * AIR_JITTER_MAX_PLANE;
    L.meta = L.plane + sizeof(float) * GJ_ROT * GJ_ROT;
    L.total = L.meta + sizeof(int) * GJ_META_INTS;
    return L;
}

struct JitterConsts { double z0, z1, gain; };
inline JitterConsts jitter_consts() {
    JitterConsts k;
    k.z0 = std::sqrt(67.5 - std::sqrt(4436.25)) + std::sqrt(26.25) - 6.5;
    k.z1 = std::sqrt(67.5 + std::sqrt(4436.25)) - std::sqrt(26.25) - 6.5;
    k.gain = (1.0 * ((1.0 - k.z0) * (1.0 - 1.0 / k.z0))) * ((1.0 - k.z1) * (1.0 - 1.0 / k.z1));
    return k;
}

// one line of the prefilter, in place: n elements, `stride` doubles apart
__device__ __forceinline__ void gj_filter_line(double* c, int n, int stride, const JitterConsts& k) {
    if (n <= 1) return;
    for (int i = 0; i < n; ++i) c[i * stride] *= k.gain;
    for (int p = 0; p < 2; ++p) {
        const double z = p == 0 ? k.z0 : k.z1;
        double zn = 1.0;
        for (int i = 0; i < n - 1; ++i) zn = zn * z;
        double c0 = c[0] + zn * c[(n - 1) * stride], zi = z;
        for (int i = 1; i < n - 1; ++i) {
            c0 = c0 + zi * (c[i * stride] + zn * c[(n - 1 - i) * stride]);
            zi = zi * z;
        }
        c[0] = c0 / (1.0 - zn * zn);
        for (int i = 1; i < n; ++i) c[i * stride] = c[i * stride] + z * c[(i - 1) * stride];
        c[(n - 1) * stride] = ((z * c[(n - 2) * stride] + c[(n - 1) * stride]) * z) / (z * z - 1.0);
        for (int i = n - 2; i >= 0; --i) c[i * stride] = z * (c[(i + 1) * stride] - c[i * stride]);
    }
}

__device__ __forceinline__ double gj_w_outer(double y) {
    return y * (y * (y * (y * (y / 24.0 - 0.375) + 1.25) - 1.75) + 0.625) + 0.425;
}
__device__ __forceinline__ double gj_w_inner(double y) {
    const double t = y * y;
    return t * (t * (0.25 - y / 12.0) - 0.5) + 0.55;
}
// the weights of the taps floor - 2 .. floor + 3 at fraction x
__device__ __forceinline__ void gj_weights(double x, double& w0, double& w1, double& w2, double& w3, double& w4, double& w5) {
    const double y = 1.0 - x, t = y * y;
    w2 = gj_w_inner(x);
    w3 = gj_w_inner(y);
    w0 = y * t * t / 120.0;
    w1 = gj_w_outer(x + 1.0);
    w4 = gj_w_outer(2.0 - x);
    w5 = 1.0 - ((((w0 + w1) + w2) + w3) + w4);
}

// tap index i (any integer) on a line of n, mirrored with period 2n - 2
__device__ __forceinline__ int gj_mirror(int i, int n) {
    if (n == 1) return 0;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

// One stage, by the whole workgroup.  In: the box (bx, by, bw, bh) of `plane` (row stride ps).  Out: plane [OH, OW] (row
// stride OW) = the transform with matrix (m00 m01; m10 m11) and offset (offy, offx), thresholded; box[0..3] = min x, min y,
// max x, max y of its pixels > 0 (box was initialised to (INT_MAX, INT_MAX, -1, -1) behind an earlier barrier).  Ends behind
// a barrier.  1 <= bw, bh <= 48 and 1 <= OH, OW <= 64 are the caller's checks.
__device__ __forceinline__ void gj_stage(double* coef, float* plane, int* box, int ps, int bx, int by, int bw, int bh, int OH,
                                         int OW, double m00, double m01, double m10, double m11, double offy, double offx,
                                         const JitterConsts& k) {
    const int tid = threadIdx.x;
    for (int p = tid; p < bh * bw; p += GJ_THREADS) {
        const int py = p / bw, px = p - py * bw;
        coef[p] = (double)plane[(by + py) * ps + bx + px];
    }
    __syncthreads();
    if (tid < bw) gj_filter_line(coef + tid, bh, bw, k);              // axis 0: thread t has column t
    __syncthreads();
    if (tid < bh) gj_filter_line(coef + tid * bw, bw, 1, k);          // axis 1: thread t has row t
    __syncthreads();                                                  // (also: every read of the old plane is done)
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int p = tid; p < OH * OW; p += GJ_THREADS) {
        const int oy = p / OW, ox = p - oy * OW;
        const double cy = ((double)oy * m00 + (double)ox * m01) + offy, cx = ((double)oy * m10 + (double)ox * m11) + offx;
        float r = 0.0f;
        if (!(cy < 0.0 || cy > (double)(bh - 1) || cx < 0.0 || cx > (double)(bw - 1))) {
            const double fy = floor(cy), fx = floor(cx);
            double wy[6], wx[6];
            gj_weights(cy - fy, wy[0], wy[1], wy[2], wy[3], wy[4], wy[5]);
            gj_weights(cx - fx, wx[0], wx[1], wx[2], wx[3], wx[4], wx[5]);
            const int iy = (int)fy - 2, ix = (int)fx - 2;
            int mx[6];
#pragma unroll
            for (int kx = 0; kx < 6; ++kx) mx[kx] = gj_mirror(ix + kx, bw);
            double t = 0.0;
#pragma unroll
            for (int ky = 0; ky < 6; ++ky) {
                const double* row = coef + gj_mirror(iy + ky, bh) * bw;
#pragma unroll
                for (int kx = 0; kx < 6; ++kx) t = t + (row[mx[kx]] * wy[ky]) * wx[kx];
            }
            r = (float)t;
            r = fminf(fmaxf(r, 0.0f), 1.0f);
            if (r < 0.05f) r = 0.0f;
        }
        plane[p] = r;
        if (r > 0.0f) {
            x0 = ox < x0 ? ox : x0; x1 = ox > x1 ? ox : x1;
            y0 = oy < y0 ? oy : y0; y1 = oy > y1 ? oy : y1;
        }
    }
    if (x1 >= 0) {                                                    // (LDS atomics; no thread waits on another's)
        atomicMin(&box[0], x0); atomicMin(&box[1], y0);
        atomicMax(&box[2], x1); atomicMax(&box[3], y1);
    }
    __syncthreads();
}

__global__ __launch_bounds__(GJ_THREADS) void glyph_jitter_kernel(air_glyph_jitter_t a, JitterConsts k, size_t off_plane,
                                                                  size_t off_meta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gj_lds[];
    double* coef = reinterpret_cast<double*>(gj_lds);
    float* plane = reinterpret_cast<float*>(gj_lds + off_plane);
    int* meta = reinterpret_cast<int*>(gj_lds + off_meta);
    const int tid = threadIdx.x, v = blockIdx.x, gd = a.gd, od = a.od;

    // the draws of one variant (at most 7 words: two quads)
    AirDraws<GJ_SALT> d((uint32_t)v, (uint32_t)(a.counter ? *a.counter : (int64_t)0), a.seed);
    const int g = d.range(0, a.G);
    const bool scaled = a.min_w != 1.0 || a.max_w != 1.0 || a.min_h != 1.0 || a.max_h != 1.0;
    const bool rotated = a.min_ang != 0.0 || a.max_ang != 0.0;
    double nw = 1.0, nh = 1.0, ang = 0.0, c = 1.0, s = 0.0;
    if (scaled) {
        nw = d.real(a.min_w, a.max_w);
        nh = d.real(a.min_h, a.max_h);
    }
    if (rotated) {
        ang = d.real(a.min_ang, a.max_ang);
        // |ang| <= 180: q = the nearest multiple of 90, r = ang - 90 q exactly, |r| <= 45; cos, sin of r by sincospi
        const double q = rint(ang / 90.0), r = ang - 90.0 * q;
        double sr, cr;
        sincospi(r / 180.0, &sr, &cr);
        const int qi = (int)q & 3;
        c = qi == 0 ? cr : qi == 1 ? -sr : qi == 2 ? -cr : sr;
        s = qi == 0 ? sr : qi == 1 ? cr : qi == 2 ? -sr : -cr;
    }

    if (tid < GJ_META_INTS) meta[tid] = (tid & 3) < 2 ? INT_MAX : -1;
    // the image so far: the box (bx, by, bw, bh) of `plane`, row stride ps; first the base glyph's crop
    const int4 base = *reinterpret_cast<const int4*>(a.crops + (size_t)g * 4);
    int bx = 0, by = 0, bw = base.z, bh = base.w, ps = base.z;
    int status = bw >= 1 && bh >= 1 && base.x >= 0 && base.y >= 0 && base.x + bw <= gd && base.y + bh <= gd ? 0 : 1;
    if (status == 0) {
        const float* src = a.glyphs + (size_t)g * gd * gd;
        for (int p = tid; p < bh * bw; p += GJ_THREADS) {
            const int py = p / bw, px = p - py * bw;
            plane[p] = src[(base.y + py) * gd + base.x + px];
        }
    }
    __syncthreads();

    if (status == 0 && scaled) {
        const double fh = (double)gd * nh, fw = (double)gd * nw;
        if (!(fh >= 1.0 && fw >= 1.0 && fh < (double)(AIR_JITTER_MAX_PLANE + 1) && fw < (double)(AIR_JITTER_MAX_PLANE + 1)))
            status = 2;
        else {
            const int OH = (int)fh, OW = (int)fw;
            gj_stage(coef, plane, meta, ps, bx, by, bw, bh, OH, OW, 1.0 / nh, 0.0, 0.0, 1.0 / nw, 0.0, 0.0, k);
            if (meta[2] < 0) status = 1;
            else { bx = meta[0]; by = meta[1]; bw = meta[2] - bx + 1; bh = meta[3] - by + 1; ps = OW; }
        }
    }
    if (status == 0 && rotated) {
        const double hh = (double)bh, ww = (double)bw;
        const double r01 = s * ww, r02 = c * hh, r03 = c * hh + s * ww, r11 = c * ww, r12 = (-s) * hh, r13 = (-s) * hh + c * ww;
        const double lo0 = fmin(fmin(0.0, r01), fmin(r02, r03)), hi0 = fmax(fmax(0.0, r01), fmax(r02, r03));
        const double lo1 = fmin(fmin(0.0, r11), fmin(r12, r13)), hi1 = fmax(fmax(0.0, r11), fmax(r12, r13));
        const double fh = (hi0 - lo0) + 0.5, fw = (hi1 - lo1) + 0.5;
        if (!(fh >= 1.0 && fw >= 1.0 && fh < (double)(GJ_ROT + 1) && fw < (double)(GJ_ROT + 1)))
            status = 2;
        else {
            const int OH = (int)fh, OW = (int)fw;
            const double ca = ((double)OH - 1.0) / 2.0, cb = ((double)OW - 1.0) / 2.0;
            const double offy = (hh - 1.0) / 2.0 - (c * ca + s * cb), offx = (ww - 1.0) / 2.0 - ((-s) * ca + c * cb);
            gj_stage(coef, plane, meta + 4, ps, bx, by, bw, bh, OH, OW, c, s, -s, c, offy, offx, k);
            if (meta[6] < 0) status = 1;
            else { bx = meta[4]; by = meta[5]; bw = meta[6] - bx + 1; bh = meta[7] - by + 1; ps = OW; }
        }
    }
    if (status == 0 && (bw > od || bh > od)) status = 2;

    float* out = a.bank + (size_t)v * od * od;
    for (int p = tid; p < od * od; p += GJ_THREADS) {
        const int py = p / od, px = p - py * od;
        out[p] = status == 0 && py < bh && px < bw ? plane[(by + py) * ps + bx + px] : 0.0f;
    }
    if (tid == 0) {
        *reinterpret_cast<int4*>(a.bank_crops + (size_t)v * 4) = status == 0 ? make_int4(0, 0, bw, bh) : make_int4(0, 0, 0, 0);
        a.source[v] = g;
        a.status[v] = status;
    }
    if (tid < 6)
        a.params[(size_t)v * 6 + tid] = tid == 0 ? nw : tid == 1 ? nh : tid == 2 ? ang : tid == 3 ? c : tid == 4 ? s : 0.0;
}

// floor(gd * bound) as the kernel's int(gd * new_height) sees it at that bound
inline double jitter_side(int gd, double bound) { return std::floor((double)gd * bound); }

int jitter_check_sizes(int gd, int od) {
    if (gd < 1 || od < 1 || od < gd) return AIR_EINVAL;
    if (gd > AIR_SCENE_MAX_GLYPH || od > AIR_SCENE_MAX_GLYPH) return AIR_ELIMIT;
    return 0;
}

// an invalid size before a limit, a limit before a null pointer
int jitter_check(const air_glyph_jitter_t* a) {
    if (!a) return AIR_EINVAL;
    if (a->V < 1 || a->G < 1 || a->gd < 1 || a->od < 1 || a->od < a->gd) return AIR_EINVAL;
    const double b[6] = {a->min_w, a->max_w, a->min_h, a->max_h, a->min_ang, a->max_ang};
    for (double x : b) if (!std::isfinite(x)) return AIR_EINVAL;
    if (a->min_w > a->max_w || a->min_h > a->max_h || a->min_ang > a->max_ang) return AIR_EINVAL;
    if (a->min_w <= 0.0 || a->min_h <= 0.0) return AIR_EINVAL;
    if (jitter_side(a->gd, a->min_h) < 1.0 || jitter_side(a->gd, a->min_w) < 1.0) return AIR_EINVAL;
    if (int rc = jitter_check_sizes(a->gd, a->od)) return rc;
    if (jitter_side(a->gd, a->max_h) > AIR_JITTER_MAX_PLANE || jitter_side(a->gd, a->max_w) > AIR_JITTER_MAX_PLANE) return AIR_ELIMIT;
    if (std::fabs(a->min_ang) > 180.0 || std::fabs(a->max_ang) > 180.0) return AIR_ELIMIT;
    if (!a->glyphs || !a->crops || !a->bank || !a->bank_crops || !a->source || !a->params || !a->status) return AIR_EINVAL;
    if (((uintptr_t)a->crops & 15) || ((uintptr_t)a->bank_crops & 15)) return AIR_EALIGN;    // a crop box is one 16-byte access
    if ((uintptr_t)a->params & 7) return AIR_EALIGN;
    return 0;
}

}  // namespace

extern "C" int64_t air_glyph_jitter_lds(int gd, int od) {
    if (int rc = jitter_check_sizes(gd, od)) return rc;
    return (int64_t)jitter_lds(gd, od).total;
}

extern "C" int air_glyph_jitter_prepare(const air_glyph_jitter_t* a) { return jitter_check(a); }

extern "C" int air_glyph_jitter(const air_glyph_jitter_t* a, void* stream) {
    if (int rc = jitter_check(a)) return rc;
    const JitterLds L = jitter_lds(a->gd, a->od);
    hipLaunchKernelGGL(glyph_jitter_kernel, dim3(a->V), dim3(GJ_THREADS), L.total, air_stream(stream), *a, jitter_consts(),
                       L.plane, L.meta);
    AIR_CHECK_LAUNCH();
    return 0;
}
