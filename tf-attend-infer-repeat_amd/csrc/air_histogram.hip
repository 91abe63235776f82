// TensorFlow 1.3's HistogramSummary (core/lib/histogram/histogram.cc) of up to AIR_HISTOGRAM_MAX strided 2-D views in one
// call: see the "histogram summaries" section of air_hip.h for the semantics and the output layout.
//
// Three kernels on the caller's stream, no synchronisation, no floating-point atomics:
//   hist_zero_kernel   zeroes the dense count arrays of all records (the caller's buffers may hold garbage; the counts are
//                      merged with integer atomics, so they need a zero to start from);
//   hist_kernel        one workgroup per work item = (histogram, chunk of HG_CHUNK elements of its row-major index space) --
//                      the 2756 x 1024 LSTM kernel and a one-element bias share one grid.  Counts in LDS (integer
//                      ds_add, non-returning), merged into the record with integer global atomics (order-free, hence the
//                      same bits every time); min / max / num / sum / sum_squares / nonfinite of the chunk go to the
//                      workspace: fp64 sums per thread in element order, a fixed wave butterfly, the waves in order;
//   hist_final_kernel  one wave per histogram adds the chunk records -- lane i those of chunks i, i + 64, ... in ascending order,
//                      then a fixed butterfly: one order, whatever the scheduling -- and writes the six doubles.
//
// Bucket index without fp64 work per element.  The limits are +-(1e-12 * 1.1^j) and 0.  For an fp32 value a >= 0 and a
// double limit P:  P <= a  <=>  ceil32(P) <= a  and  P < a  <=>  above32(P) <= a, with ceil32(P) the smallest fp32 not below P
// and above32(P) the smallest fp32 strictly above it (the two differ only where P is itself an fp32).  Both tables are built
// at COMPILE time from the same double loop the host function runs, staged in LDS, and searched from a first guess off
// log2(a) (the limits are geometric) that two comparison loops correct: the result is exact whatever the guess.
//   x >= 0 (and -0.0):  bucket = POS + 1 + #{j : ceil32(P_j) <= x}
//   x <  0, a = -x:     bucket = POS - #{j : above32(P_j) <= a}
#include "air_common.h"
#include <float.h>

namespace {

constexpr int HG_THREADS = 512;                 // (1024 threads cap the kernel at 128 VGPRs, which the compiler then spills)
constexpr int HG_CHUNK = 8192;                   // elements per work item (a multiple of 4: the 16-byte path never splits a group)

constexpr int hg_positive_limits() {
    int n = 0;
    for (double v = 1e-12; v < 1e20; v *= 1.1) ++n;
    return n + 1;                                // ... and DBL_MAX
}
constexpr int HG_POS = hg_positive_limits();     // 775
constexpr int HG_BUCKETS = 2 * HG_POS + 1;       // 1551
constexpr int HG_COUNT_WORDS = (HG_BUCKETS + 1) & ~1;                   // the counts of a record, padded to 8 bytes
constexpr int64_t HG_RECORD_BYTES = 6 * 8 + 4 * (int64_t)HG_COUNT_WORDS;

struct HgTables { float le[HG_POS]; float lt[HG_POS]; };
constexpr float hg_next_up(float f) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + 1u); }   // f > 0, finite
constexpr HgTables hg_make_tables() {
    HgTables t{};
    int j = 0;
    for (double v = 1e-12; v < 1e20; v *= 1.1, ++j) {
        float f = (float)v;                                  // nearest ...
        if ((double)f < v) f = hg_next_up(f);                // ... made the ceiling
        t.le[j] = f;
        t.lt[j] = (double)f == v ? hg_next_up(f) : f;
    }
    t.le[j] = t.lt[j] = __builtin_inff();                    // DBL_MAX: above every finite fp32
    return t;
}
__device__ const HgTables hg_tables = hg_make_tables();

struct HgParams {
    air_histogram_desc_t d[AIR_HISTOGRAM_MAX];
    int32_t chunk0[AIR_HISTOGRAM_MAX + 1];       // first work item of each histogram; [count] = their number
    int32_t count;
    float prescale;
    const float* dyn;
    const float* gnorm;
    unsigned char* out;
    double* ws;                                  // [work items][6]: min, max, num, sum, sum_squares, nonfinite
};
static_assert(sizeof(HgParams) <= 4096, "kernel arguments");

__device__ __forceinline__ uint32_t* hg_counts(unsigned char* out, int h) {
    return reinterpret_cast<uint32_t*>(out + (int64_t)h * HG_RECORD_BYTES + 48);
}

__global__ __launch_bounds__(HG_THREADS) void hist_zero_kernel(unsigned char* out, int count) {
    const int n = count * HG_COUNT_WORDS;
    for (int i = blockIdx.x * HG_THREADS + threadIdx.x; i < n; i += gridDim.x * HG_THREADS)
        hg_counts(out, i / HG_COUNT_WORDS)[i % HG_COUNT_WORDS] = 0u;
}

// float order as unsigned order (-0.0 below +0.0), from the bits alone: no comparison depends on the denormal mode
__device__ __forceinline__ uint32_t hg_key(uint32_t b) { return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__device__ __forceinline__ float hg_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

struct HgAcc {
    double sum, sq;
    uint32_t mn, mx, num, bad;
};

__device__ __forceinline__ void hg_add(float x, int kind, float sc, const float* tab, uint32_t* cnt, HgAcc& acc) {
    const float y = kind ? x * sc : x;
    const uint32_t b = __float_as_uint(y), ab = b & 0x7fffffffu;
    if (ab >= 0x7f800000u) { ++acc.bad; return; }
    const float a = __uint_as_float(ab);
    const bool neg = (b >> 31) != 0u && ab != 0u;
    const float* T = tab + (neg ? HG_POS : 0);
    // P_j = 1e-12 * 1.1^j  ->  j ~ (log2 a + log2 1e12) / log2 1.1; a zero or flushed denormal gives -inf -> 0
    float gf = (__log2f(a) + 39.863137f) * 7.2725408f;
    gf = fminf(fmaxf(gf, 0.0f), (float)(HG_POS - 1));
    int g = (int)gf;
    while (g < HG_POS - 1 && T[g] <= a) ++g;                 // T[HG_POS - 1] = +inf is never <= a
    while (g > 0 && T[g - 1] > a) --g;
    atomicAdd(&cnt[neg ? HG_POS - g : HG_POS + 1 + g], 1u);
    const double yd = (double)y;
    acc.sum += yd;
    acc.sq += yd * yd;
    const uint32_t k = hg_key(b);
    acc.mn = min(acc.mn, k);
    acc.mx = max(acc.mx, k);
    ++acc.num;
}

__global__ __launch_bounds__(HG_THREADS) void hist_kernel(const HgParams p) {
    __shared__ uint32_t cnt[HG_BUCKETS];
    __shared__ float tab[2 * HG_POS];
    __shared__ double red_d[HG_THREADS / 64][2];
    __shared__ uint32_t red_u[HG_THREADS / 64][4];
    const int tid = threadIdx.x, blk = blockIdx.x;
    int lo = 0, hi = p.count;                                // the histogram of this work item: chunk0[lo] <= blk < chunk0[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.chunk0[mid] <= blk) lo = mid; else hi = mid;
    }
    const int h = lo;
    const air_histogram_desc_t d = p.d[h];
    const int64_t n = (int64_t)d.rows * d.cols;
    const int64_t e0 = (int64_t)(blk - p.chunk0[h]) * HG_CHUNK;
    const int len = (int)(n - e0 < HG_CHUNK ? n - e0 : HG_CHUNK);
    const int64_t row0 = e0 / d.cols;
    const uint32_t col0 = (uint32_t)(e0 - row0 * d.cols), cols = (uint32_t)d.cols;
    float sc = 1.0f;
    if (d.scale_kind == 1) sc = p.prescale;
    else if (d.scale_kind == 2) {                            // AirAdamCoef.scale of air_common.h, the same expression
        const float clip = p.dyn[AIR_DYN_CLIP_NORM], gnorm = p.gnorm[0];
        sc = p.prescale * (clip > 0.0f ? clip * fminf(1.0f / gnorm, 1.0f / clip) : 1.0f);
    }
    for (int i = tid; i < HG_BUCKETS; i += HG_THREADS) cnt[i] = 0u;
    for (int i = tid; i < HG_POS; i += HG_THREADS) { tab[i] = hg_tables.le[i]; tab[HG_POS + i] = hg_tables.lt[i]; }
    __syncthreads();

    HgAcc acc = {0.0, 0.0, 0xffffffffu, 0u, 0u, 0u};
    const bool vec = (d.cols & 3) == 0 && (d.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(d.base) & 15) == 0;
    if (vec) {                                               // n, e0, col0 and len are multiples of 4: a group never leaves its row
#pragma unroll 1
        for (int k = 4 * tid; k < len; k += 4 * HG_THREADS) {
            const uint32_t c = col0 + (uint32_t)k, r = c / cols;
            const float4 v = *reinterpret_cast<const float4*>(d.base + (row0 + r) * (int64_t)d.ld + (c - r * cols));
            hg_add(v.x, d.scale_kind, sc, tab, cnt, acc);
            hg_add(v.y, d.scale_kind, sc, tab, cnt, acc);
            hg_add(v.z, d.scale_kind, sc, tab, cnt, acc);
            hg_add(v.w, d.scale_kind, sc, tab, cnt, acc);
        }
    } else {
#pragma unroll 1
        for (int k = tid; k < len; k += HG_THREADS) {
            const uint32_t c = col0 + (uint32_t)k, r = c / cols;
            hg_add(d.base[(row0 + r) * (int64_t)d.ld + (c - r * cols)], d.scale_kind, sc, tab, cnt, acc);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.sum += __shfl_xor(acc.sum, off, 64);
        acc.sq += __shfl_xor(acc.sq, off, 64);
        acc.mn = min(acc.mn, (uint32_t)__shfl_xor((int)acc.mn, off, 64));
        acc.mx = max(acc.mx, (uint32_t)__shfl_xor((int)acc.mx, off, 64));
        acc.num += (uint32_t)__shfl_xor((int)acc.num, off, 64);
        acc.bad += (uint32_t)__shfl_xor((int)acc.bad, off, 64);
    }
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        red_d[w][0] = acc.sum; red_d[w][1] = acc.sq;
        red_u[w][0] = acc.mn; red_u[w][1] = acc.mx; red_u[w][2] = acc.num; red_u[w][3] = acc.bad;
    }
    __syncthreads();                                         // ... and every LDS count of the chunk is in
    uint32_t* gc = hg_counts(p.out, h);
    for (int i = tid; i < HG_BUCKETS; i += HG_THREADS) {
        const uint32_t c = cnt[i];
        if (c) atomicAdd(&gc[i], c);
    }
    if (tid == 0) {
        double sum = red_d[0][0], sq = red_d[0][1];
        uint32_t mn = red_u[0][0], mx = red_u[0][1], num = red_u[0][2], bad = red_u[0][3];
        for (int w = 1; w < HG_THREADS / 64; ++w) {
            sum += red_d[w][0]; sq += red_d[w][1];
            mn = min(mn, red_u[w][0]); mx = max(mx, red_u[w][1]); num += red_u[w][2]; bad += red_u[w][3];
        }
        double* o = p.ws + (int64_t)blk * 6;
        o[0] = num ? (double)hg_unkey(mn) : (double)__builtin_inff();
        o[1] = num ? (double)hg_unkey(mx) : -(double)__builtin_inff();
        o[2] = (double)num; o[3] = sum; o[4] = sq; o[5] = (double)bad;
    }
}

__global__ __launch_bounds__(64) void hist_final_kernel(const HgParams p) {
    const int h = blockIdx.x, tid = threadIdx.x, c0 = p.chunk0[h], c1 = p.chunk0[h + 1];
    double mn = (double)__builtin_inff(), mx = -(double)__builtin_inff(), num = 0.0, sum = 0.0, sq = 0.0, bad = 0.0;
    for (int c = c0 + tid; c < c1; c += 64) {                // lane i: chunks i, i + 64, ... in ascending order
        const double* w = p.ws + (int64_t)c * 6;
        mn = fmin(mn, w[0]); mx = fmax(mx, w[1]);
        num += w[2]; sum += w[3]; sq += w[4]; bad += w[5];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                 // ... then the fixed butterfly: one order, the same bits every time
        mn = fmin(mn, __shfl_xor(mn, off, 64)); mx = fmax(mx, __shfl_xor(mx, off, 64));
        num += __shfl_xor(num, off, 64); sum += __shfl_xor(sum, off, 64);
        sq += __shfl_xor(sq, off, 64); bad += __shfl_xor(bad, off, 64);
    }
    if (tid == 0) {
        double* o = reinterpret_cast<double*>(p.out + (int64_t)h * HG_RECORD_BYTES);
        o[0] = mn; o[1] = mx; o[2] = num; o[3] = sum; o[4] = sq; o[5] = bad;
    }
}

// the one reading of the descriptors: every entry point answers from it, before any HIP call
int hg_plan(const air_histogram_desc_t* descs, int count, HgParams* p, int64_t* items) {
    if (!descs || count < 1) return AIR_EINVAL;
    if (count > AIR_HISTOGRAM_MAX) return AIR_ELIMIT;
    int64_t total = 0;
    for (int h = 0; h < count; ++h) {
        const air_histogram_desc_t& d = descs[h];
        if (!d.base || d.rows < 1 || d.cols < 1 || d.ld < d.cols || d.scale_kind < 0 || d.scale_kind > 2) return AIR_EINVAL;
    }
    for (int h = 0; h < count; ++h) {
        const air_histogram_desc_t& d = descs[h];
        if (reinterpret_cast<uintptr_t>(d.base) & 3) return AIR_EALIGN;
        const int64_t n = (int64_t)d.rows * d.cols;
        if (n > 0xffffffffll) return AIR_ELIMIT;             // the counts are uint32
        if (p) { p->d[h] = d; p->chunk0[h] = (int32_t)total; }
        total += (n + HG_CHUNK - 1) / HG_CHUNK;
    }
    if (p) { p->chunk0[count] = (int32_t)total; p->count = count; }
    *items = total;                                          // <= 128 * 2^18
    return 0;
}

}  // namespace

extern "C" int air_histogram_num_buckets(void) { return HG_BUCKETS; }
extern "C" int air_histogram_chunk(void) { return HG_CHUNK; }
extern "C" int64_t air_histogram_record_bytes(void) { return HG_RECORD_BYTES; }

extern "C" int air_histogram_limits(double* out) {
    if (!out) return AIR_EINVAL;
    double pos[HG_POS];
    int n = 0;
    for (double v = 1e-12; v < 1e20; v *= 1.1) pos[n++] = v;
    pos[n++] = DBL_MAX;
    for (int i = 0; i < n; ++i) { out[i] = -pos[n - 1 - i]; out[n + 1 + i] = pos[i]; }
    out[n] = 0.0;
    return 0;
}

extern "C" int64_t air_histograms_output_bytes(const air_histogram_desc_t* descs, int count) {
    int64_t items;
    const int rc = hg_plan(descs, count, nullptr, &items);
    return rc ? rc : count * HG_RECORD_BYTES;
}

extern "C" int64_t air_histograms_workspace_bytes(const air_histogram_desc_t* descs, int count) {
    int64_t items;
    const int rc = hg_plan(descs, count, nullptr, &items);
    return rc ? rc : items * 48;
}

extern "C" int air_histograms(const air_histograms_t* a, void* stream) {
    if (!a) return AIR_EINVAL;
    HgParams p = {};
    int64_t items;
    const int rc = hg_plan(a->descs, a->count, &p, &items);
    if (rc) return rc;
    if (!a->out || !a->workspace) return AIR_EINVAL;
    for (int h = 0; h < a->count; ++h)
        if (a->descs[h].scale_kind == 2 && (!a->dyn || !a->gnorm)) return AIR_EINVAL;
    if (a->out_bytes < a->count * HG_RECORD_BYTES || a->workspace_bytes < items * 48) return AIR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(a->out) | reinterpret_cast<uintptr_t>(a->workspace)) & 7) return AIR_EALIGN;
    p.prescale = a->prescale;
    p.dyn = a->dyn;
    p.gnorm = a->gnorm;
    p.out = static_cast<unsigned char*>(a->out);
    p.ws = static_cast<double*>(a->workspace);
    hipStream_t s = air_stream(stream);
    const int zero_blocks = (a->count * HG_COUNT_WORDS + HG_THREADS - 1) / HG_THREADS;
    hipLaunchKernelGGL(hist_zero_kernel, dim3(zero_blocks), dim3(HG_THREADS), 0, s, p.out, a->count);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(hist_kernel, dim3((unsigned)items), dim3(HG_THREADS), 0, s, p);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(hist_final_kernel, dim3(a->count), dim3(64), 0, s, p);
    AIR_CHECK_LAUNCH();
    return 0;
}
