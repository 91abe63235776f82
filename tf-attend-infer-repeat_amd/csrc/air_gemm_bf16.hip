// bf16-TWIN operand GEMM (precision 1 when the caller supplies bf16 twins of the operands).
//
// The fp32-operand kernel of air_gemm.hip (gemm_bf16v2_kernel) rounds both operand panels to bf16 on
// their way into LDS: every workgroup pulls 4-byte elements through its CU's L1 and spends most of its
// VALU instructions on v_cvt_pk_bf16_f32 and on transposing row-major weights into k-contiguous
// fragments.  Here the operands ARE bf16 in memory -- the producing epilogue / the Adam step wrote an
// RNE-rounded twin next to every fp32 array (air_gemm_t.A16 / B16) -- so
//   * a k-contiguous operand (activations; weights of a data-gradient GEMM, transB) is copied
//     global -> VGPR -> LDS in 16-byte pieces of 8 k, one ds_write_b128 into the same XOR-swizzled
//     [row][64 k] image the fp32-operand kernel builds: half the bytes, half the load instructions,
//     no conversion;
//   * an n-contiguous operand (row-major [K,N] weights of a forward GEMM) is copied AS IT LIES into a
//     [64 k][BN] image (lane-linear 16-byte stores, conflict free) and its MFMA fragments are read
//     with gfx950's transpose read ds_read_b64_tr_b16: each 16-lane group fetches a [4 k][16 n] block
//     and every lane receives the 4 k of its own column (semantics and bank behaviour measured in
//     tools/exp/tr_read.hip) -- two of them give the 8 consecutive k v_mfma_f32_16x16x32_bf16 wants.
//     No VALU instruction touches the operand;
//   * the number of 64-deep images per round R is a template parameter picked from K, so a K = 256
//     product does not issue (masked) loads for images it does not have, and K <= 1024 is ONE round.
// The rounding is the RNE the other kernel applies on the way into LDS, accumulation order over k,
// cross-wave reduction and epilogues are shared code (air_gemm_common.h): results are bit-identical to
// the fp32-operand bf16 path (tests/test_gpu_kernels.py::test_gemm_bf16_twins_bit_identical).
// A may stay fp32 (AF32: the hoisted x.Wx reads the caller's fp32 image batch).  That launch can leave a PADDED bf16
// twin of the batch behind (row stride K rounded up to 8 elements: every row starts 16-byte aligned, pad columns
// zero); the x.Wx launches that follow it over the same batch read the twin -- half the A bytes -- and fill both LDS
// images by 16-byte LDS-DMA (gemm_xwx_glds_kernel below).
#include "air_gemm_common.h"
#include <atomic>
#include <cstdlib>
#include <cstdio>

using namespace airg;

AIR_STAMPS_READER(air_debug_stamps_gemm_tw)

namespace {

__device__ __forceinline__ uint4 ldg16u(const char* base, unsigned off, bool ok) {
    const uint4 t = *reinterpret_cast<const uint4*>(base + (ok ? off : 0u));
    return ok ? t : make_uint4(0u, 0u, 0u, 0u);
}
__device__ __forceinline__ uint2 ldg8u(const char* base, unsigned off, bool ok) {
    const uint2 t = *reinterpret_cast<const uint2*>(base + (ok ? off : 0u));
    return ok ? t : make_uint2(0u, 0u);
}
__device__ __forceinline__ float4 ldg16f(const char* base, unsigned off, bool ok) {
    const float4 t = *reinterpret_cast<const float4*>(base + (ok ? off : 0u));
    return ok ? t : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int TM, int TN, int R>
struct TwCfg {
    static constexpr int BM = 16 * TM, BN = 16 * TN, KB = 64;
    static constexpr int IMG = (BM + BN) * KB * 2;                       // bytes per image pair
    static constexpr int RED = 3 * TM * TN * 4 * 64 * 4;                 // bytes of the cross-wave reduction
    static constexpr int BYTES = (R * IMG > RED) ? R * IMG : RED;
};

template <int TM, int TN, bool TB, int EPI_, bool AF32, int R>
__global__ __launch_bounds__(THREADS) void gemm_bf16tw_kernel(Args a)
{
    using Cfg = TwCfg<TM, TN, R>;
    constexpr int BM = Cfg::BM, BN = Cfg::BN, KB = Cfg::KB;
    extern __shared__ __attribute__((aligned(16))) unsigned char Lds[];   // Cfg::BYTES
    unsigned short* ImgA = reinterpret_cast<unsigned short*>(Lds);       // [R][BM][64], 16-byte slots swizzled by row
    unsigned short* ImgB = ImgA + R * BM * KB;                           // TB: [R][BN][64] swizzled; else [R][64][BN]
    float* Red = reinterpret_cast<float*>(Lds);

    if (prologue_plane(a)) return;
    constexpr bool QUAD = quad_epi(EPI_);                  // 16 columns = 4 gates x 4 units (TN == 1, untransposed B)
    const Frame f = frame_of<TM, TN, QUAD>(a);
    const int nslab = f.nslab, zslab = f.zslab, tid = f.tid, lane = f.lane, wave = f.wave, m0 = f.m0, n0 = f.n0, kbeg = f.kbeg, kend = f.kend;

    AIR_STAMP(56);
    f32x4 acc[TM][TN];
    zero_acc(acc);

    Pre<TM, TN> pre;

    const char* Ab = AF32 ? reinterpret_cast<const char*>(a.A) : reinterpret_cast<const char*>(a.A16);
    // B from its panel-blocked twin when the caller has one (untransposed B only): a 16-column tile's rows are then
    // 32 contiguous bytes each, consecutive k contiguous -- whole cache lines instead of a quarter (plain panels) or
    // a sixteenth (four 8-byte gate pieces per row of a row-major LSTM kernel) of every line pulled through the CU
    const bool pnl = !TB && a.B16p != nullptr;
    const char* Bb = reinterpret_cast<const char*>(pnl ? a.B16p : a.B16);
    const unsigned pK16 = (unsigned)a.K * 16u;
    // tasks of one round, 16 bytes each.  k-contiguous bf16 operand: (image, row, slot g of 8 k) -- eight
    // consecutive lanes read one whole 128-byte row of an image.  fp32 A: (image, row, 4 k), rounded on the
    // way into LDS as the fp32-operand kernel does.  n-contiguous B: (image, k, 8 columns).
    constexpr int TA_N = AF32 ? (R * BM * 16 + THREADS - 1) / THREADS : (R * BM * 8 + THREADS - 1) / THREADS;
    constexpr int TBK_N = (R * BN * 8 + THREADS - 1) / THREADS;
    constexpr int TBN_N = (R * KB * (BN / 8) + THREADS - 1) / THREADS;
    constexpr int TBQ_N = (R * KB * 4 + THREADS - 1) / THREADS;           // QUAD: (image, k, gate) -> 8 bytes = 4 units
    // x.Wx on the gate-interleaved PANEL twin: the tile's block is contiguous, so it travels in 16-byte pieces of two gates
    // (half the load instructions, the same bytes in the same registers: piece i = vq[2 i], vq[2 i + 1]); wave-uniform
    const bool quad16 = EPI_ == AIR_EPI_LSTM_FWD0 && pnl;
    constexpr int TBQ16_N = (TBQ_N + 1) / 2;
    uint4 va[AF32 ? 1 : TA_N];
    float4 vaf[AF32 ? TA_N : 1];
    uint4 vb[QUAD ? 1 : (TB ? TBK_N : TBN_N)];
    uint2 vq[QUAD ? 2 * TBQ16_N : 1];
    // AF32 x.Wx: the workgroups of column panel 0 leave their rows behind as the padded bf16 twin (a.C16, row stride ldt)
    const bool twin_out = AF32 && EPI_ == AIR_EPI_LSTM_FWD0 && a.C16 != nullptr && n0 == 0;
    const int ldt = (a.K + 7) & ~7;

    auto issue_loads = [&](int kr) __attribute__((always_inline)) {
        if (AF32) {
#pragma unroll
            for (int i = 0; i < TA_N; ++i) {
                const int u = tid + THREADS * i;
                const int c = u / (BM * 16), row = (u / 16) % BM, hh = u & 15;
                const int gm = m0 + row, gk = kr + c * KB + hh * 4;
                const bool ok = (u < R * BM * 16) && gm < a.M && gk < kend;
                vaf[i] = ldg16f(Ab, ((unsigned)gm * (unsigned)a.lda + (unsigned)gk) * 4u, ok);
            }
        } else {
#pragma unroll
            for (int i = 0; i < TA_N; ++i) {
                const int u = tid + THREADS * i;
                const int c = u / (BM * 8), row = (u / 8) % BM, g = u & 7;
                const int gm = m0 + row, gk = kr + c * KB + g * 8;
                const bool ok = (u < R * BM * 8) && gm < a.M && gk < kend;
                va[i] = ldg16u(Ab, ((unsigned)gm * (unsigned)a.lda + (unsigned)gk) * 2u, ok);
            }
        }
        if (QUAD && quad16) {
#pragma unroll
            for (int i = 0; i < TBQ16_N; ++i) {
                const int t = tid + THREADS * i;
                const int gk = kr + (t >> 1);
                const bool ok = (t < R * KB * 2) && n0 < a.gwidth && gk < kend;
                const uint4 v = ldg16u(Bb, ((unsigned)(n0 >> 2) * pK16 + (unsigned)kr * 16u) * 2u + (unsigned)t * 16u, ok);
                vq[2 * i] = make_uint2(v.x, v.y); vq[2 * i + 1] = make_uint2(v.z, v.w);
            }
        } else if (QUAD) {
#pragma unroll
            for (int i = 0; i < TBQ_N; ++i) {
                const int t = tid + THREADS * i;
                const int c = t / (KB * 4), k = (t >> 2) % KB, gate = t & 3;
                const int gn = group_col<true>(a, n0, gate * 4).gn, gk = kr + c * KB + k;
                const bool ok = (t < R * KB * 4) && n0 < a.gwidth && gk < kend;
                const unsigned off = pnl ? (unsigned)(n0 >> 2) * pK16 + (unsigned)gk * 16u + (unsigned)gate * 4u
                                         : (unsigned)gk * (unsigned)a.ldb + (unsigned)gn;
                vq[i] = ldg8u(Bb, off * 2u, ok);
            }
        } else if (TB) {
#pragma unroll
            for (int i = 0; i < TBK_N; ++i) {
                const int u = tid + THREADS * i;
                const int c = u / (BN * 8), col = (u / 8) % BN, g = u & 7;
                const GroupCol gc = group_col(a, n0, col);
                const int gk = kr + c * KB + g * 8;
                const bool ok = (u < R * BN * 8) && gc.cg < a.gwidth && gc.gn < a.N && gk < kend;
                vb[i] = ldg16u(Bb, ((unsigned)gc.gn * (unsigned)a.ldb + (unsigned)gk) * 2u, ok);
            }
        } else {
#pragma unroll
            for (int i = 0; i < TBN_N; ++i) {
                const int t = tid + THREADS * i;
                const int c = t / (KB * (BN / 8)), k = (t / (BN / 8)) % KB, h = t % (BN / 8);
                const GroupCol gc = group_col(a, n0, h * 8);
                const int gk = kr + c * KB + k;
                const bool ok = (t < R * KB * (BN / 8)) && gc.cg < a.gwidth && gc.gn < a.N && gk < kend;
                const unsigned off = pnl ? (unsigned)(gc.gn >> 4) * pK16 + (unsigned)gk * 16u + (unsigned)(gc.gn & 15)
                                         : (unsigned)gk * (unsigned)a.ldb + (unsigned)gc.gn;
                vb[i] = ldg16u(Bb, off * 2u, ok);
            }
        }
    };
    // (tried: a mask-free form for interior tiles / full passes -- one per-thread base address, uniform pass offsets.
    // In-kernel stamps: the issue phase of the K = 256 kernels 0.84 -> 0.56 us, nothing at K = 784, and the in-graph
    // launch times did not move (the phase is bound by the CU's vector-memory path -- 64 B/clk, and a 16-column tile
    // uses 32 bytes of every 128-byte line of a row-major weight -- not by its ~15 VALU instructions per piece))
    auto store_images = [&](int kr) __attribute__((always_inline)) {
        if (AF32) {
#pragma unroll
            for (int i = 0; i < TA_N; ++i) {
                const int u = tid + THREADS * i;
                const int c = u / (BM * 16), row = (u / 16) % BM, hh = u & 15;
                uint2 w;
                w.x = air_pack_bf16(vaf[i].x, vaf[i].y); w.y = air_pack_bf16(vaf[i].z, vaf[i].w);
                if (u < R * BM * 16)
                    *reinterpret_cast<uint2*>(&ImgA[(c * BM + row) * KB + (((hh >> 1) ^ (row & 7)) << 3) + (hh & 1) * 4]) = w;
                if (twin_out) {                       // (block-uniform) columns K .. ldt - 1 were loaded as zeros: the pad
                    const int gm = m0 + row, gk = kr + c * KB + hh * 4;
                    if (u < R * BM * 16 && gm < a.M && gk < ldt)
                        *reinterpret_cast<uint2*>(&a.C16[(size_t)gm * ldt + gk]) = w;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < TA_N; ++i) {
                const int u = tid + THREADS * i;
                const int c = u / (BM * 8), row = (u / 8) % BM, g = u & 7;
                if (u < R * BM * 8) *reinterpret_cast<uint4*>(&ImgA[(c * BM + row) * KB + ((g ^ (row & 7)) << 3)]) = va[i];
            }
        }
        if (QUAD && quad16) {
#pragma unroll
            for (int i = 0; i < TBQ16_N; ++i) {
                const int t = tid + THREADS * i;
                if (t < R * KB * 2)                                                         // the same image, two gates a piece
                    *reinterpret_cast<uint4*>(&ImgB[t * 8]) = make_uint4(vq[2 * i].x, vq[2 * i].y, vq[2 * i + 1].x, vq[2 * i + 1].y);
            }
        } else if (QUAD) {
#pragma unroll
            for (int i = 0; i < TBQ_N; ++i) {
                const int t = tid + THREADS * i;
                if (t < R * KB * 4) *reinterpret_cast<uint2*>(&ImgB[t * 4]) = vq[i];           // [c][k][gate][4 units]: lane-linear
            }
        } else if (TB) {
#pragma unroll
            for (int i = 0; i < TBK_N; ++i) {
                const int u = tid + THREADS * i;
                const int c = u / (BN * 8), col = (u / 8) % BN, g = u & 7;
                if (u < R * BN * 8) *reinterpret_cast<uint4*>(&ImgB[(c * BN + col) * KB + ((g ^ (col & 7)) << 3)]) = vb[i];
            }
        } else {
#pragma unroll
            for (int i = 0; i < TBN_N; ++i) {
                const int t = tid + THREADS * i;
                if (t < R * KB * (BN / 8)) *reinterpret_cast<uint4*>(&ImgB[t * 8]) = vb[i];      // [c][k][BN]: lane-linear
            }
        }
    };

    issue_loads(kbeg);
    // the epilogue's operands ride behind the first round's panels (same memory round trip)
    if (nslab == 1) epilogue_prefetch<TM, TN, EPI_>(a, pre, m0, n0, lane, wave);
    AIR_STAMP(57);
    for (int kr = kbeg; kr < kend; kr += R * KB) {
        if (kr > kbeg) __syncthreads();                                   // images of the previous round consumed
        store_images(kr);
        if (kr + R * KB < kend) issue_loads(kr + R * KB);
        __syncthreads();
        AIR_STAMP(58);
        // ---- MFMAs: mfma_round_bf16<TM, TN, R, !TB> (air_gemm_common.h), left inline HERE: through the function the
        // register allocation of the 32 x 32 tiles with R = 8 changes -- same instructions, 164 -> 188 VGPRs, occupancy
        // 3 -> 2 in <2, 2, false, 0, false, 8>.  Keep the two in step.
        const int cfirst = (wave - ((kr - kbeg) / KB)) & 3;
#pragma unroll
        for (int cc = 0; cc < (R + 3) / 4; ++cc) {
            const int c = cfirst + 4 * cc;
            if (c < R && kr + c * KB < kend) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int slot = ks * 4 + (lane >> 4);
                    bf16x8 av[TM], bv[TN];
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        const int row = i * 16 + (lane & 15);
                        av[i] = *reinterpret_cast<const bf16x8*>(&ImgA[(c * BM + row) * KB + ((slot ^ (row & 7)) << 3)]);
                    }
                    if (TB) {
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const int col = j * 16 + (lane & 15);
                            bv[j] = *reinterpret_cast<const bf16x8*>(&ImgB[(c * BN + col) * KB + ((slot ^ (col & 7)) << 3)]);
                        }
                    } else {
                        const int il = lane & 15;
                        const unsigned short* blk = &ImgB[(c * KB + ks * 32 + (lane >> 4) * 8 + (il >> 2)) * BN + (il & 3) * 4];
#pragma unroll
                        for (int j = 0; j < TN; ++j) bv[j] = read_tr_bf16x8(blk + j * 16, BN);
                    }
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
                }
            }
        }
    }
    AIR_STAMP(59);
    __syncthreads();                                                      // Red aliases the images
    reduce_waves<TM, TN>(acc, Red, lane, wave);
    AIR_STAMP(60);
    if (nslab > 1) { store_slab<TM, TN>(a, Red, zslab, m0, n0, lane, wave); return; }
    epilogue<TM, TN, EPI_>(a, pre, Red, m0, n0, lane, wave);
    AIR_STAMP(61);
}


// ---------------------------------------------------------------------------
// Throughput tiling for the ONE deep contraction of a large canvas: the hoisted x.Wx of the 128x128 configuration,
// [256 x 1024 x 16384] -- fp32 image batch (the caller's tensor) x the bf16 shadow of Wx, split-K slabs out.
// The latency kernel above splits K over its four waves and re-reads the image batch once per 32/64-column tile
// (512 / 256 MB through the L1s).  Here a workgroup owns a 64 x 64 output tile, each wave a 32 x 32 quadrant of it
// over the WHOLE K slab (no cross-wave reduction), operands stream through double-buffered 64-deep LDS stages with the
// loads of FOUR stages in flight per thread and two workgroups per CU; the row panel of a (row tile, slab) pair is kept in
// one XCD's L2 for its 16 column tiles.  Interior tiles only (M % 64, N % 64, K slab % 64 == 0: the dispatcher checks).
// ---------------------------------------------------------------------------
// BN = 128 (round 4): the launch is bound by what ONE CU can pull through its L1 (~45 GB/s when every line misses it):
// with 64 x 64 tiles a CU's two workgroups read 2 x (512 KB of fp32 rows + 256 KB of bf16 columns) per slab = 1.5 MB ->
// 37 us.  A 64 x 128 tile (each wave 32 x 64) reads 512 + 512 KB for twice the outputs: 256 workgroups, one per CU, 1 MB
// each.  Same k order per accumulator: bit-identical.
template <int BN>
__global__ __launch_bounds__(THREADS) void gemm_xw_tp_kernel(Args a)
{
    constexpr int BM = 64, KB = 64, D = 4;               // D: stages of global loads in flight per thread (a memory round
                                                         // trip is ~1 us, a stage's MFMAs ~0.15 us: one stage ahead is not enough)
    constexpr int NJ = BN / 32;                          // 16-column MFMA tiles per wave (its half of the tile's columns)
    constexpr int PPR = BN / 8, RPP = THREADS / PPR, NBP = KB / RPP;    // B: 16-byte pieces per k row, rows per pass, passes
    __shared__ __attribute__((aligned(16))) unsigned short ImgA[2][BM * KB];   // [row][64 k], 16-byte slots swizzled by row
    __shared__ __attribute__((aligned(16))) unsigned short ImgB[2][KB * BN];   // [k][64 n] as it lies (transpose read)
    // the step prologue's planes of workgroups come LAST in dispatch order here: the product's 512 workgroups take their
    // CUs first and the prologue (at 128 x 128: 1.3 M quads of noise and image-twin work, 4 096 workgroups) fills in beside
    // them -- in front, it delayed the product by its whole duration (54.5 us per launch against 34 + 6 as two launches)
    const int nz = (int)gridDim.z - a.job_on;
    if ((int)blockIdx.z >= nz) {
        const long plane = (long)gridDim.x * gridDim.y;
        air_step_job_run(a.job, ((int)blockIdx.z - nz) * plane + (long)blockIdx.y * gridDim.x + blockIdx.x, plane * a.job_on);
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware map (workgroup b runs on XCD b % 8, each XCD with its own 4 MB L2).  Round 3 kept all column tiles of a
    // (row tile, slab) pair on one XCD: the fp32 A panel of the pair came from memory once -- but the four row tiles that
    // share a B panel (the bf16 shadow of Wx: 33.5 MB, the BIGGER operand) then sat on four different XCDs, and the
    // counters showed it: 167 MB read for 50 MB of operands.  Now a K SLAB is an XCD's: all (row tile, column tile) pairs
    // of slab z run on XCD z % 8, stepping through k together (two workgroups per CU, 64 per XCD at the stress shape), so
    // every line of BOTH operands is fetched from memory by one L2 only and its other users hit there.
    // (The old map was an environment switch until ABI 4 removed it.)
    int tile_m = blockIdx.y, tile_n = blockIdx.x, zslab = (int)blockIdx.z;
    {
        const int nx = gridDim.x, ny = gridDim.y, pairs = ny * nz;
        const int lin = (zslab * ny + (int)blockIdx.y) * nx + (int)blockIdx.x;
        const int xcd = lin & 7, slot = lin >> 3;
        if (a.i1 == 0 && (nz & 7) == 0) {
            zslab = xcd + 8 * (slot / (nx * ny));
            const int rem = slot % (nx * ny);
            tile_n = rem % nx; tile_m = rem / nx;
        } else if ((pairs & 7) == 0) {
            const int pair = xcd + 8 * (slot / nx);
            tile_n = slot % nx; tile_m = pair % ny; zslab = pair / ny;
        }
    }
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int kbeg = zslab * a.kslab, kend = min(a.K, kbeg + a.kslab);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * (BN / 2);   // this wave's 32 x BN/2 part, over the whole K slab

    f32x4 acc[2][NJ];
    zero_acc(acc);

    // staging maps: A piece = float4 (4 k) of row (tid >> 4) + 16 i; B piece = 16 bytes (8 columns) of k row tid / PPR + RPP i
    const int ar = tid >> 4, ah = tid & 15, bk = tid / PPR, bh = tid % PPR;
    const float* pa = a.A + (size_t)(m0 + ar) * a.lda + ah * 4;
    const unsigned short* pb = a.B16 + (size_t)bk * a.ldb + n0 + bh * 8;
    const unsigned la = ar * KB + (((ah >> 1) ^ (ar & 7)) << 3) + (ah & 1) * 4;      // (row + 16 i) & 7 == ar & 7
    typedef float f32v4 __attribute__((ext_vector_type(4)));
    typedef unsigned u32v4 __attribute__((ext_vector_type(4)));
    f32v4 va[D][4];                                       // (native vector types: the HIP structs kept this ring in scratch)
    u32v4 vb[D][NBP];
    // (the ring slot is a compile-time constant everywhere -- std::integral_constant -- so that the ring lives in
    // registers: with a run-time slot index the arrays went to scratch memory, 39.8 -> 54.6 us)
    auto load_stage = [&](auto dc, int k0) __attribute__((always_inline)) {
        constexpr int d = decltype(dc)::value;
#pragma unroll
        for (int i = 0; i < 4; ++i) va[d][i] = *reinterpret_cast<const f32v4*>(pa + (size_t)(16 * i) * a.lda + k0);
#pragma unroll
        for (int i = 0; i < NBP; ++i) vb[d][i] = *reinterpret_cast<const u32v4*>(pb + (size_t)(k0 + RPP * i) * a.ldb);
    };
    int buf = 0;
    auto stage = [&](auto dc, int k0) __attribute__((always_inline)) {
        constexpr int d = decltype(dc)::value;
        if (k0 >= kend) return;                            // (uniform)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint2 w;
            w.x = air_pack_bf16(va[d][i].x, va[d][i].y); w.y = air_pack_bf16(va[d][i].z, va[d][i].w);
            *reinterpret_cast<uint2*>(&ImgA[buf][la + 16 * i * KB]) = w;
        }
#pragma unroll
        for (int i = 0; i < NBP; ++i) *reinterpret_cast<u32v4*>(&ImgB[buf][(bk + RPP * i) * BN + bh * 8]) = vb[d][i];
        if (k0 + D * KB < kend) load_stage(dc, k0 + D * KB);        // refill this ring slot: D stages ahead
        __syncthreads();                                  // (also: everyone is past the MFMAs of the stage that used the other buffer)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int slot = ks * 4 + (lane >> 4), il = lane & 15;
            bf16x8 av[2], bv[NJ];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int row = wm + i * 16 + il;
                av[i] = *reinterpret_cast<const bf16x8*>(&ImgA[buf][row * KB + ((slot ^ (row & 7)) << 3)]);
            }
            const unsigned short* blk = &ImgB[buf][(ks * 32 + (lane >> 4) * 8 + (il >> 2)) * BN + wn + (il & 3) * 4];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bv[j] = read_tr_bf16x8(blk + j * 16, BN);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        buf ^= 1;
    };
    using I0 = std::integral_constant<int, 0>; using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>; using I3 = std::integral_constant<int, 3>;
    static_assert(D == 4, "ring depth");
    if (kbeg < kend) load_stage(I0{}, kbeg);
    if (kbeg + KB < kend) load_stage(I1{}, kbeg + KB);
    if (kbeg + 2 * KB < kend) load_stage(I2{}, kbeg + 2 * KB);
    if (kbeg + 3 * KB < kend) load_stage(I3{}, kbeg + 3 * KB);
    for (int kb = kbeg; kb < kend; kb += D * KB) {
        stage(I0{}, kb); stage(I1{}, kb + KB); stage(I2{}, kb + 2 * KB); stage(I3{}, kb + 3 * KB);
    }
    float* Cz = a.C + (size_t)zslab * a.slab_stride;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Cz[(size_t)(m0 + wm + i * 16 + (lane >> 4) * 4 + q) * a.ldc + n0 + wn + j * 16 + (lane & 15)] = acc[i][j][q];
}

// ---------------------------------------------------------------------------
// The hoisted x.Wx + first LSTM step over the PADDED bf16 twin of the image batch (a.A16, row stride a.lda a
// multiple of 8 elements) and the gate-interleaved panel twin of Wx (a.B16p): the 16 x 16 tile, the 64-deep images,
// the image -> wave map, the reduction and the epilogue of gemm_bf16tw_kernel<1, 1, false, AIR_EPI_LSTM_FWD0, .., R>,
// with both LDS images filled by 16-byte LDS-DMA (global_load_lds_dwordx4: no staging VGPR, no ds_write pass).
// An LDS-DMA wave instruction writes 64 x 16 bytes lane-linear from a wave-uniform base, so
//   * B: the tile's panel block [k][gate][4 units] is contiguous in memory and its image is that block: piece t of a
//     round goes to byte 16 t;
//   * A: the image is [row][64 k] with the 16-byte slots of a row XOR-swizzled by row & 7.  Piece u = (image, row,
//     slot g) is WRITTEN at byte 16 u and FETCHES slot g ^ (row & 7) of its row -- a permutation inside one 128-byte
//     line, the same involution the fragment reads apply (tests/test_xwx_twin_swizzle.py);
//   * a piece outside the matrix (rows >= M, k >= K) is not fetched: its lane writes the zeros itself (ds_write), so
//     the images hold what register staging puts there.
// One barrier per round; __syncthreads() waits for the fills (they count on vmcnt).
// ---------------------------------------------------------------------------
template <int R>
__global__ __launch_bounds__(THREADS) void gemm_xwx_glds_kernel(Args a)
{
    using Cfg = TwCfg<1, 1, R>;
    constexpr int BM = 16, BN = 16, KB = 64;
    constexpr int EPI_ = AIR_EPI_LSTM_FWD0;
    extern __shared__ __attribute__((aligned(16))) unsigned char Lds[];   // Cfg::BYTES
    unsigned short* ImgA = reinterpret_cast<unsigned short*>(Lds);       // [R][16][64], slots swizzled by row
    unsigned short* ImgB = ImgA + R * BM * KB;                           // [R][64][4 gates][4 units]
    float* Red = reinterpret_cast<float*>(Lds);
    typedef __attribute__((address_space(3))) unsigned char lds_u8;
    typedef const __attribute__((address_space(1))) unsigned char glb_u8;

    if (prologue_plane(a)) return;
    const Frame f = frame_of<1, 1, true>(a);
    const int tid = f.tid, lane = f.lane, wave = f.wave, m0 = f.m0, n0 = f.n0;
    const int kbeg = 0, kend = a.K;                      // one slab (twin_rounds)

    f32x4 acc[1][1];
    zero_acc(acc);
    Pre<1, 1> pre;

    const char* Ab = reinterpret_cast<const char*>(a.A16);
    const char* Bb = reinterpret_cast<const char*>(a.B16p) + (size_t)(n0 >> 2) * (size_t)a.K * 32u;
    constexpr int TA_N = R * BM * 8 / THREADS, TB_N = R * KB * 2 / THREADS;
    static_assert((R * BM * 8) % THREADS == 0 && (R * KB * 2) % THREADS == 0, "whole passes of 16-byte pieces");
    lds_u8* const lA = (lds_u8*)Lds;
    lds_u8* const lB = lA + R * BM * KB * 2;
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    // a pass = 256 pieces = two images of A / 128 k of B; what a thread fetches differs from pass to pass by a constant
    const int arow = (tid >> 3) & 15, asg = (tid & 7) ^ (arow & 7);       // (u / 8) % 16, and the slot FETCHED for slot u & 7
    const int ka = (tid >> 7) * KB + asg * 8, kb = tid >> 1;              // this thread's k within a pass
    const bool arow_ok = m0 + arow < a.M;
    const int lim_a = arow_ok ? kend : 0, lim_b = n0 < a.gwidth ? kend : 0;
    const char* const pa = Ab + ((size_t)(arow_ok ? m0 + arow : 0) * (size_t)a.lda + (size_t)ka) * 2u;
    const char* const pb = Bb + tid * 16;
    const int wbase = __builtin_amdgcn_readfirstlane(wave) * 1024;        // the wave's 64 x 16 bytes of a pass (scalar: it goes to M0)

    // the zeros first, all of them, then the fills: a ds_write behind an LDS-DMA in flight would wait for it (vmcnt(0))
    auto fill_images = [&](int kr) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TA_N; ++i)
            if (__builtin_expect(!(kr + 2 * KB * i + ka < lim_a), 0)) *reinterpret_cast<uint4*>(&ImgA[(tid + THREADS * i) * 8]) = zero4;
#pragma unroll
        for (int i = 0; i < TB_N; ++i)
            if (__builtin_expect(!(kr + 2 * KB * i + kb < lim_b), 0)) *reinterpret_cast<uint4*>(&ImgB[(tid + THREADS * i) * 8]) = zero4;
#pragma unroll
        for (int i = 0; i < TA_N; ++i)
            if (__builtin_expect(kr + 2 * KB * i + ka < lim_a, 1))
                __builtin_amdgcn_global_load_lds((glb_u8*)(pa + (size_t)(kr + 2 * KB * i) * 2u), lA + wbase + THREADS * 16 * i, 16, 0, 0);
#pragma unroll
        for (int i = 0; i < TB_N; ++i)
            if (__builtin_expect(kr + 2 * KB * i + kb < lim_b, 1))
                __builtin_amdgcn_global_load_lds((glb_u8*)(pb + (size_t)(kr + 2 * KB * i) * 32u), lB + wbase + THREADS * 16 * i, 16, 0, 0);
    };

    AIR_STAMP(56);
    fill_images(kbeg);
    epilogue_prefetch<1, 1, EPI_>(a, pre, m0, n0, lane, wave);
    AIR_STAMP(57);
    for (int kr = kbeg; kr < kend; kr += R * KB) {
        if (kr > kbeg) { __syncthreads(); fill_images(kr); }              // images of the previous round consumed
        __syncthreads();
        AIR_STAMP(58);
        mfma_round_bf16<1, 1, R, true>(acc, ImgA, ImgB, kr, kbeg, kend, lane, wave);
        if (R >= 40) break;                                               // (twin_rounds: 40 images are the whole contraction)
    }
    AIR_STAMP(59);
    __syncthreads();                                                      // Red aliases the images
    reduce_waves<1, 1>(acc, Red, lane, wave);
    AIR_STAMP(60);
    epilogue<1, 1, EPI_>(a, pre, Red, m0, n0, lane, wave);
    AIR_STAMP(61);
}

// every bf16-twin kernel instantiation, once: (template arguments) -> (function, dynamic LDS bytes)
#define TW(TM_, TN_, TB_, EPI__, AF_, R_)                                                                               \
    {{BF16TW, TM_, TN_, false, TB_, EPI__, AF_, R_}, reinterpret_cast<const void*>(&gemm_bf16tw_kernel<TM_, TN_, TB_, EPI__, AF_, R_>), \
     TwCfg<TM_, TN_, R_>::BYTES}
#define GLDS(R_) {{XWX_GLDS, 1, 1, false, false, AIR_EPI_LSTM_FWD0, false, R_}, reinterpret_cast<const void*>(&gemm_xwx_glds_kernel<R_>), TwCfg<1, 1, R_>::BYTES}
#define TP(BN_) {{XW_TP, 8, 4, false, false, AIR_EPI_GENERIC, false, BN_}, reinterpret_cast<const void*>(&gemm_xw_tp_kernel<BN_>), 0}
const Kern TWIN_KERNELS[] = {
    // the hoisted x.Wx carrying the first LSTM step: fp32 or twin A, register or (padded twin A) LDS-DMA staging
    TW(1, 1, false, AIR_EPI_LSTM_FWD0, true, 16), TW(1, 1, false, AIR_EPI_LSTM_FWD0, true, 40),
    TW(1, 1, false, AIR_EPI_LSTM_FWD0, false, 16), TW(1, 1, false, AIR_EPI_LSTM_FWD0, false, 40), GLDS(16), GLDS(40),
    TW(1, 1, false, AIR_EPI_GENERIC, false, 4), TW(1, 1, false, AIR_EPI_GENERIC, false, 8), TW(1, 1, false, AIR_EPI_GENERIC, false, 16),
    TW(1, 1, true, AIR_EPI_GENERIC, false, 4), TW(1, 1, true, AIR_EPI_GENERIC, false, 8), TW(1, 1, true, AIR_EPI_GENERIC, false, 16),
    TW(1, 1, true, AIR_EPI_LSTM_BWD, false, 4), TW(1, 1, true, AIR_EPI_LSTM_BWD, false, 8), TW(1, 1, true, AIR_EPI_LSTM_BWD, false, 16),
    TW(1, 1, true, AIR_EPI_LSTM_BWD_TAIL, false, 4), TW(1, 1, true, AIR_EPI_LSTM_BWD_TAIL, false, 8), TW(1, 1, true, AIR_EPI_LSTM_BWD_TAIL, false, 16),
    // AIR_EPI_LSTM_FWD: 16-column tiles of four units x four gates (8-byte pieces of 4 units)
    TW(1, 1, false, EPI_LSTM_FWD_Q, false, 4),
    TW(2, 2, false, AIR_EPI_GENERIC, true, 8), TW(2, 2, false, AIR_EPI_GENERIC, false, 4), TW(2, 2, false, AIR_EPI_GENERIC, false, 8),
    TW(2, 2, true, AIR_EPI_GENERIC, false, 4), TW(2, 2, true, AIR_EPI_GENERIC, false, 8),
    TW(4, 2, false, AIR_EPI_GENERIC, true, 4), TW(4, 2, false, AIR_EPI_GENERIC, false, 4),
    TW(4, 4, false, AIR_EPI_GENERIC, true, 4), TW(4, 4, false, AIR_EPI_GENERIC, false, 4),
    // tile (8, 4) of the ABI = the throughput kernel (128 x 64 or 64 x 128 per workgroup, quadrant per wave)
    TP(64), TP(128)};
#undef TW
#undef GLDS
#undef TP

}  // namespace

const Kern* airg::twin_kernels(int& n) {
    n = (int)(sizeof(TWIN_KERNELS) / sizeof(TWIN_KERNELS[0]));
    return TWIN_KERNELS;
}

namespace {

// fp32 -> bf16 (RNE) copy: the twin of an array its producer could not write (variables after a
// host-side load; Adam keeps the shadow fresh afterwards)
__global__ __launch_bounds__(256) void bf16_twin_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, long n) {
    const long n4 = n / 4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(src)[i];
        reinterpret_cast<uint2*>(dst)[i] = make_uint2(air_pack_bf16(v.x, v.y), air_pack_bf16(v.z, v.w));
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - n4 * 4)) dst[n4 * 4 + threadIdx.x] = air_bf16_of(src[n4 * 4 + threadIdx.x]);
}

}  // namespace

extern "C" int air_bf16_twin(const float* src, uint16_t* dst, int64_t n, void* stream) {
    if (!src || !dst || n <= 0) return AIR_EINVAL;
    if (!aligned16(src) || !aligned8(dst)) return AIR_EALIGN;
    long blocks = (n / 4 + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
    hipLaunchKernelGGL(bf16_twin_kernel, dim3((unsigned)blocks), dim3(256), 0, air_stream(stream), src, dst, (long)n);
    AIR_CHECK_LAUNCH();
    return 0;
}
