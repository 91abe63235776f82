// Grouped weight-gradient launch: every dW = A^T . dY of the train step (the MatMul_grad / BiasAdd_grad nodes of all 36
// variables) in ONE kernel.  Device code first, the host's table and the entry points behind it.
//
// Weights are shared across the N time steps, so each dW contracts over all N*B (step, image) rows: K is small (64 ..
// 256; 1280 and more for the stress canvases and the gathered factors) while M x N is the size of the weight matrix -- an
// outer-product-shaped GEMM.  A 64 x 64 output tile is owned by one workgroup; its 4 waves own disjoint 32 x 32 quadrants
// and run the full K loop themselves (no split-K, no cross-wave reduction).  The problems of the step are independent:
// one launch (Table: up to MAXP problems, found by workgroup number) fills the chip instead of ten latency-bound ones.
//
// What a workgroup runs:
//   tile_f32      precision 0 (wgrad_grouped_kernel): fp32 operands in 32-row chunks through two LDS buffers, all loads
//                 of up to 6 chunks issued before the first is consumed, v_mfma_f32_16x16x4f32.
//   tile_bf16     precision 1 (wgrad_grouped_bf16_kernel), fp32 operands: rounded to bf16 on their way into [column][k]
//                 LDS images, up to three 64-row images per round, v_mfma_f32_16x16x32_bf16.
//   tile_bf16_tw  precision 1, both operands have usable bf16 twins (twin_ok): the twins are copied as they lie into
//                 [k][64] images and read through gfx950's transpose read.  Bit-identical to tile_bf16.
//   run_strip_bf16  precision 1, twins, a problem of >= 512 tiles with K in {64, 128, 192, 256} (strip_of): one workgroup
//                 owns 2 or 4 consecutive column tiles of a block-row, keeps the A fragments in registers and streams the
//                 dY tiles.  Bit-identical to one tile per workgroup.
//   run_bias_wg   either precision, K >= 384: the launch's FIRST workgroups sum one 64-column block of db each.
// Every tile leaves LDS through store_tile (whole 256-byte rows per store instruction) and publishes the sum of squares of
// what it stored as one global-norm partial (publish_sq).
//
// Who owns a bias column.  db[n0 .. n0 + 63] and its squares belong to exactly ONE workgroup: a bias workgroup when
// K >= 384; else the tile (or strip) of the column in block-row 0, or in block-row nt % bias_mod for the problems of >= 512
// tiles (owns_bias) -- decided by shape alone, so both precisions and every operand path of a problem agree.  The column
// sums are always taken from the fp32 dY (A for the head units), before any rounding.
//
// Order of the partials: one per 64 x 64 tile, problems in table order, tiles of a problem row-major (Prob::first_part +
// tile number, whoever computes the tile: a strip publishes one per tile at the tile's own index); behind all tiles one
// per bias workgroup, in launch order (Prob::bias_part).  The Adam kernel re-reduces them in that fixed order.
#include "air_common.h"
#include "air_mfma.h"
#include <type_traits>
#include <cstring>
#include <cstdlib>

namespace airw {

using airm::f32x4; using airm::bf16x8;
using airm::zero_acc; using airm::read_tr_bf16x8; using airm::aligned16; using airm::aligned8;      // air_mfma.h

constexpr int THREADS = 256;
constexpr int BT = 64;          // output tile (both dims)
constexpr int KC = 32;          // rows per staged chunk (fp32 tile)
constexpr int LS = BT + 16;     // LDS row stride: = 16 (mod 32) dwords -> conflict-free fragment reads, 16-B aligned
constexpr int KB = 64;          // rows per LDS image (bf16 tiles)
constexpr int NIMG_W = 3;       // images resident per round in the bf16 tiles: K <= 192 needs one round
constexpr int MAXP = AIR_MAX_WGRAD_PROBLEMS;

struct Prob {
    const float* A; const float* dY; float* dW; float* db;
    const unsigned short* A16; const unsigned short* dY16;      // bf16 twins of A / dY (nullable): see tile_bf16_tw
    int M, N, K, lda, ldb, ldc;
    int head_pack, Hs, Hh, Hz;
    int tiles_n, first_block;   // first_block: first WORKGROUP of the problem in the grouped launch
    int first_part;             // first global-norm partial (= tile number: one partial per 64 x 64 tile, whoever computes it)
    int strip;                  // > 0: a workgroup owns `strip` consecutive column tiles of one block-row (run_strip_bf16)
    int bias_mod;               // which block-row sums db of column tile nt: 0 -> block-row 0; else block-row nt % bias_mod
    int bias_first, bias_part;  // >= 0: db is summed by workgroups OF ITS OWN (run_bias_wg), one per column tile -- their first
                                // workgroup in the launch and their first global-norm partial; -1: by the tiles (owns_bias)
};
// db[n0 .. n0 + 63] (and its share of the global norm) belongs to ONE tile of the column.  Block-row 0 for ordinary problems;
// for the big ones (>= 512 tiles, by shape alone -- so every precision / operand path of a problem agrees and the partials
// stay bit-identical between them) the owners are spread over the first block-rows: sixteen column sums in block-row 0
// were the long pole of a strip launch (a strip workgroup of block-row 0 summed all of its columns: +12 us at 4 tiles).
__device__ __forceinline__ bool owns_bias(const Prob& pr, int m0, int n0) {
    if (pr.bias_first >= 0) return false;
    const int nt = n0 / BT, mb = m0 / BT;
    return pr.bias_mod > 0 ? (mb == nt % pr.bias_mod) : (mb == 0);
}
// first[i] = first workgroup of problem i (INT_MAX past `count`): kept apart from the descriptors so that
// ONE wide scalar load fetches all of them and the owner is found without a chain of dependent loads
// (total_blocks = tiles = global-norm partials; launch_blocks = workgroups of the grouped launch: fewer when a problem
// runs in strips)
// nbias: the launch's first workgroups, which sum bias columns of the long-contraction problems (run_bias_wg)
struct Table { int count; int total_blocks; int launch_blocks; int nbias; int first[MAXP]; Prob p[MAXP]; };

// Rows of a bf16 twin (leading dimension ld, in elements) start 16-byte / 8-byte aligned: the twin tiles copy them in
// pieces of that size (twin_ok, tile_bf16_tw, the strip dispatch; strip_of on the host)
__host__ __device__ __forceinline__ bool rows16(const void* p, int ld) { return (ld & 7) == 0 && aligned16(p); }
__host__ __device__ __forceinline__ bool rows8(const void* p, int ld) { return (ld & 3) == 0 && aligned8(p); }

// One float4 of a row-major operand, zero outside [rows x cols], in two branch-free halves: fetch4
// issues the load(s) with out-of-range accesses redirected to element 0, mask4 zeroes what was out of
// range.  Callers issue ALL fetches of a batch before the first mask: a run-time branch around a
// load (or a consumer right behind it) makes the compiler wait on the spot, which serialises the
// 16-24 loads a thread should have in flight (12 us instead of 3 for the ragged-edge tiles).
// VEC: base 16-byte aligned and ld % 4 == 0 -- a quad that starts inside a row then lies inside
// the padded row, so the 16-byte load is issued even when its last columns are past `cols`.
template <bool VEC>
__device__ __forceinline__ float4 fetch4(const float* __restrict__ base, int ld, int row, int col, int rows, int cols) {
    const bool okr = row < rows;
    const unsigned at = (unsigned)row * (unsigned)ld + (unsigned)col;
    if (VEC) return *reinterpret_cast<const float4*>(base + ((okr && col < cols) ? at : 0u));
    float4 v;
    v.x = base[(okr && col < cols) ? at : 0u];
    v.y = base[(okr && col + 1 < cols) ? at + 1u : 0u];
    v.z = base[(okr && col + 2 < cols) ? at + 2u : 0u];
    v.w = base[(okr && col + 3 < cols) ? at + 3u : 0u];
    return v;
}
__device__ __forceinline__ float4 mask4(float4 t, int row, int col, int rows, int cols) {
    const bool okr = row < rows;
    float4 v;
    v.x = (okr && col < cols) ? t.x : 0.f;
    v.y = (okr && col + 1 < cols) ? t.y : 0.f;
    v.z = (okr && col + 2 < cols) ? t.z : 0.f;
    v.w = (okr && col + 3 < cols) ? t.w : 0.f;
    return v;
}

// ---- the parts the tiles share

// The accumulators of the four waves -> the 64 x 64 fp32 tile at Ct (rows of LS floats).  C/D map: row = (lane >> 4) * 4
// + q, col = lane & 15.  The tile goes through LDS so that every store instruction of the epilogue touches whole 256-byte
// rows (full cache lines).  The caller puts a barrier on either side.
__device__ __forceinline__ void acc_to_lds(const f32x4 (&acc)[2][2], float* Ct, int wm, int wn, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                Ct[(wm + i * 16 + (lane >> 4) * 4 + q) * LS + wn + j * 16 + (lane & 15)] = acc[i][j][q];
}

// one k-step (32 rows) of a wave's 32 x 32 quadrant: 2 x 2 MFMAs
__device__ __forceinline__ void mfma_2x2(f32x4 (&acc)[2][2], const bf16x8 (&av)[2], const bf16x8 (&bv)[2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
}

// Column sums held per (k-run g = lane & 7, column quad): sum_kruns is the xor-tree over the 8 k-runs (lanes g = 0 .. 7
// are contiguous), every lane ends with the total; store_db writes db[c0 + j] = v[j] for c0 + j < lim and returns the
// squares of what it stored, in column order.
__device__ __forceinline__ void sum_kruns(float (&csum)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = csum[j];
        s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
        csum[j] = s;
    }
}
__device__ __forceinline__ float store_db(float* db, const float (&v)[4], int c0, int lim) {
    float sq = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (c0 + j < lim) { db[c0 + j] = v[j]; sq += v[j] * v[j]; }
    return sq;
}

// sum of squares of everything this workgroup stored (tf.global_norm terms): one partial per
// workgroup, reduced again in fixed order by the Adam kernel; workgroup 0 also counts the step
// (apply_gradients(global_step=...), air_model.py:692-694).  sq_red: 4 floats of LDS supplied by the kernel
__device__ __forceinline__ void publish_sq(float sq, float* sq_partials, int32_t* istate, int part, float* sq_red) {
    sq = air_block_sum_256(sq, sq_red);
    if (threadIdx.x == 0) {
        sq_partials[part] = sq;
        if (part == 0 && istate) istate[AIR_IST_GLOBAL_STEP] += 1;
    }
}
// The same partial off the workgroup's chain (bf16 launch), in two halves with air_block_sum_256's order of additions:
// park_sq leaves each wave's sum in its own word of `red` -- words nothing else has used, so no barrier stands in front;
// publish_parked, behind ONE barrier of the caller, adds the four in wave order and stores.  A one-tile workgroup parks
// in sq_red (behind the images: the output tile does not alias it), a strip parks every tile in words of its own while
// the next tile is staged and publishes them all behind its last tile's stores.
__device__ __forceinline__ void park_sq(float sq, float* red) {
    sq = air_wave_sum(sq);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
}
__device__ __forceinline__ void publish_parked(const float* red, float* sq_partials, int32_t* istate, int part) {
    sq_partials[part] = ((red[0] + red[1]) + red[2]) + red[3];
    if (part == 0 && istate) istate[AIR_IST_GLOBAL_STEP] += 1;
}

// Epilogue of the weight-gradient kernels: the tile in Ct goes to pr.dW (whole rows per store
// instruction) and its sum of squares to the caller.  pr.dW == NULL: nothing is stored, only the
// sum of squares is taken (a gradient its caller rebuilds from the factors elsewhere).
__device__ __forceinline__ float store_tile(const Prob& pr, int m0, int n0, const float* Ct, float sq)
{
    const int tid = threadIdx.x;
    const int M = pr.M, N = pr.N, ldc = pr.ldc;
    float* dW = pr.dW;
    if (!pr.head_pack) {
        const bool vecC = ((ldc & 3) == 0) && aligned16(dW);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (tid >> 4) + 16 * r, col = (tid & 15) * 4;
            const int m = m0 + row, n = n0 + col;
            if (m >= M) continue;
            const float4 t = *reinterpret_cast<const float4*>(&Ct[row * LS + col]);
            float* dst = dW + (size_t)m * ldc + n;
            if (vecC && n + 3 < N) { if (dW) *reinterpret_cast<float4*>(dst) = t; sq += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w); }
            else {
                if (n < N) { if (dW) dst[0] = t.x; sq += t.x * t.x; }
                if (n + 1 < N) { if (dW) dst[1] = t.y; sq += t.y * t.y; }
                if (n + 2 < N) { if (dW) dst[2] = t.z; sq += t.z * t.z; }
                if (n + 3 < N) { if (dW) dst[3] = t.w; sq += t.w * t.w; }
            }
        }
    } else {
        // head output units (air_model.py:294-316, 376): A = d_out7 [K,8], dY = hid [K,HT];
        // unit o only owns the hidden segment of its head: dW = wout[o][n - off], db = bout[o] = sum_k d_out7[k][o]
        const int Hs = pr.Hs, Hh = pr.Hh, Hz = pr.Hz;
        for (int it = tid; it < 7 * BT; it += THREADS) {
            const int o = it / BT, col = it % BT, n = n0 + col;
            const int hd = air_out_head(o);
            const int off = air_head_off(Hs, Hh, hd);
            const int wd = air_head_wid(Hs, Hh, Hz, hd);
            if (m0 == 0 && n < N && n >= off && n < off + wd) {
                const float t = Ct[o * LS + col];
                dW[(size_t)o * ldc + (n - off)] = t;
                sq += t * t;
            }
        }
    }
    return sq;
}

__device__ __forceinline__ const Prob& find_tile(const Table& tab, int block, int& m0, int& n0) {
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAXP; ++i) pi += (block >= tab.first[i]) ? 1 : 0;
    const Prob& pr = tab.p[pi];
    const int local = block - pr.first_block;
    if (pr.strip > 0) {
        // strips: the groups of one block-row share its A block.  Workgroups go round-robin over the 8 XCDs, so block-rows
        // are dealt per XCD (every group of a block-row on the SAME XCD, back to back: one L2 fetches the A block once)
        const int groups = pr.tiles_n / pr.strip, tiles_m = (pr.M + BT - 1) / BT;
        int mb, g;
        if ((tiles_m & 7) == 0) { const int x = local & 7, s = local >> 3; mb = (s / groups) * 8 + x; g = s % groups; }
        else { mb = local / groups; g = local % groups; }
        m0 = mb * BT; n0 = g * pr.strip * BT;
        return pr;
    }
    m0 = (local / pr.tiles_n) * BT; n0 = (local % pr.tiles_n) * BT;
    return pr;
}

// ---------------------------------------------------------------------------
// fp32 tile: the 64 x 64 block (m0, n0) of pr.A^T . pr.dY, left as 64 rows of LS floats at &As[0][0]
// (barrier-synchronised).  Returns this thread's share of the squared bias gradient it stored: wave 0 of the tile that
// owns the column sums them from the dY chunk already in LDS.
// ---------------------------------------------------------------------------
template <int NCH>      // chunks of 32 rows in flight per round trip (8: K <= 256 in one)
__device__ __forceinline__ float tile_f32(const Prob& pr, int m0, int n0, float (*As)[KC * LS], float (*Bs)[KC * LS])
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;        // this wave's quadrant
    const bool vecA = ((pr.lda & 3) == 0) && aligned16(pr.A);
    const bool vecB = ((pr.ldb & 3) == 0) && aligned16(pr.dY);

    // copy the problem descriptor out of the kernel-argument table once
    const float* __restrict__ Ap = pr.A;
    const float* __restrict__ Yp = pr.dY;
    const int M = pr.M, N = pr.N, K = pr.K, lda = pr.lda, ldb = pr.ldb;
    float* db = pr.db;
    const int head_pack = pr.head_pack;

    // staging map: 32 rows x 16 float4 columns = 512 float4 per operand chunk, 2 per thread
    const int srow = tid >> 4, scol = (tid & 15) * 4;             // rows srow and srow + 16
    float4 ra[NCH][2], rb[NCH][2];
    auto fetch = [&](int set, int k0, auto vec_t) __attribute__((always_inline)) {
        constexpr bool V = decltype(vec_t)::value;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = k0 + srow + 16 * h;
            ra[set][h] = fetch4<V>(Ap, lda, k, m0 + scol, K, M);
            rb[set][h] = fetch4<V>(Yp, ldb, k, n0 + scol, K, N);
        }
    };
    // interior tile, whole chunks: nothing to clamp or mask
    const bool plain = vecA && vecB && m0 + BT <= M && n0 + BT <= N && (K % KC) == 0;
    auto fetch_plain = [&](int set, int k0) __attribute__((always_inline)) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const unsigned k = (unsigned)(k0 + srow + 16 * h);
            ra[set][h] = *reinterpret_cast<const float4*>(Ap + (k * (unsigned)lda + (unsigned)(m0 + scol)));
            rb[set][h] = *reinterpret_cast<const float4*>(Yp + (k * (unsigned)ldb + (unsigned)(n0 + scol)));
        }
    };
    auto stage = [&](int set, int buf, int k0, auto plain_t) __attribute__((always_inline)) {
        constexpr bool PL = decltype(plain_t)::value;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int k = k0 + srow + 16 * h;
            *reinterpret_cast<float4*>(&As[buf][(srow + 16 * h) * LS + scol]) = PL ? ra[set][h] : mask4(ra[set][h], k, m0 + scol, K, M);
            *reinterpret_cast<float4*>(&Bs[buf][(srow + 16 * h) * LS + scol]) = PL ? rb[set][h] : mask4(rb[set][h], k, n0 + scol, K, N);
        }
    };

    f32x4 acc[2][2];
    zero_acc(acc);
    float colsum = 0.0f;        // wave 0 of the owning tile: column n0 + lane of dY (or of A for the head units)
    const bool do_bias = (db != nullptr) && (wave == 0) && (head_pack ? (n0 == 0) : owns_bias(pr, m0, n0));

    auto compute = [&](int buf) {
        const float* as = As[buf];
        const float* bs = Bs[buf];
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            const int kk = ks * 4 + (lane >> 4);
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = as[kk * LS + wm + i * 16 + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = bs[kk * LS + wn + j * 16 + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        if (do_bias) {
            const float* cs = head_pack ? as : bs;                 // zero rows beyond K
#pragma unroll 8
            for (int k = 0; k < KC; ++k) colsum += cs[k * LS + lane];
        }
    };
    // ALL loads of up to NCH chunks are issued before the first is consumed (one memory round
    // trip), then one barrier per chunk: stage(c+1) only overwrites the buffer every wave finished
    // reading before it passed the barrier of iteration c.
    for (int ks0 = 0; ks0 < K; ks0 += NCH * KC) {
        if (ks0 > 0) __syncthreads();
        if (plain) {                            // ONE uniform branch around the whole batch of loads
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (ks0 + c * KC < K) fetch_plain(c, ks0 + c * KC);
        } else if (vecA && vecB) {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (ks0 + c * KC < K) fetch(c, ks0 + c * KC, std::true_type{});
        } else {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (ks0 + c * KC < K) fetch(c, ks0 + c * KC, std::false_type{});
        }
        if (plain) {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (ks0 + c * KC < K) {
                    stage(c, c & 1, ks0 + c * KC, std::true_type{});
                    __syncthreads();
                    compute(c & 1);
                }
        } else {
#pragma unroll
            for (int c = 0; c < NCH; ++c)
                if (ks0 + c * KC < K) {
                    stage(c, c & 1, ks0 + c * KC, std::false_type{});
                    __syncthreads();
                    compute(c & 1);
                }
        }
    }

    __syncthreads();
    acc_to_lds(acc, &As[0][0], wm, wn, lane);   // 64 x LS floats = 20 KB: spans As[0..1]
    __syncthreads();
    float bias_sq = 0.0f;
    if (do_bias) {
        if (!head_pack) { if (n0 + lane < N) { db[n0 + lane] = colsum; bias_sq = colsum * colsum; } }
        else if (lane < 7) { db[lane] = colsum; bias_sq = colsum * colsum; }
    }
    return bias_sq;
}

// ---------------------------------------------------------------------------
// bf16 tile (precision 1, fp32 operands): operands are rounded to bf16 (RNE,
// v_cvt_pk_bf16_f32) on their way into LDS, products run on
// v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  K sits on the slow (row)
// axis of both operands, the MFMA wants 8 consecutive k per lane: a thread
// loads the same 4 columns of 8 consecutive rows (8 x 16-B loads), packs one
// 16-B k-run per column and stores it into a [column][k] image whose 16-B slots
// are XOR-swizzled by the column index -- conflict-free for the 8-lane
// ds_write_b128 groups and for the 16-lane ds_read_b128 fragment groups.  All
// loads of up to 192 rows are in flight at once, one barrier before the MFMAs
// (no per-chunk barriers); the bias column sums are taken from the fp32
// registers before rounding.
// Img = [operand][image][column][k] shorts of LDS (2 x NIMG_W x 8 KB); the fp32 tile is left at its start (64 rows of LS
// floats, barrier-synchronised).
// ---------------------------------------------------------------------------
__device__ __forceinline__ float tile_bf16(const Prob& pr, int m0, int n0, unsigned short* Img)
{
    constexpr int NIMG = NIMG_W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const float* __restrict__ Ap = pr.A;
    const float* __restrict__ Yp = pr.dY;
    const int M = pr.M, N = pr.N, K = pr.K, lda = pr.lda, ldb = pr.ldb;
    float* db = pr.db;
    const int head_pack = pr.head_pack;

    // staging role: threads 0..127 own operand A, 128..255 own dY; g = k-run (8 rows), q = column quad
    const int op = tid >> 7, g = tid & 7, q = (tid & 127) >> 3;
    const float* src = op ? Yp : Ap;
    const int ld = op ? ldb : lda, cols = op ? N : M, c0 = (op ? n0 : m0) + 4 * q;
    const bool vec = ((ld & 3) == 0) && aligned16(src);
    unsigned short* img = Img + (size_t)op * NIMG * BT * KB;
    const bool bias_block = (db != nullptr) && (head_pack ? (n0 == 0) : owns_bias(pr, m0, n0));
    const bool bias_thread = bias_block && (op == (head_pack ? 0 : 1));
    float csum[4] = {0.f, 0.f, 0.f, 0.f};

    f32x4 acc[2][2];
    zero_acc(acc);

    AIR_STAMP(1);
    for (int kr = 0; kr < K; kr += NIMG * KB) {
        if (kr > 0) __syncthreads();                     // every wave is done reading the previous images
        float4 v[NIMG][8];
        // wave-uniform choices, each ONE branch around the whole batch of loads
        const bool inside = (op ? n0 : m0) + BT <= cols;                  // no ragged column edge
        if (vec && inside && (K % KB) == 0) {
            // interior tile, whole images: uniform base + 32-bit byte offsets, nothing to mask
            const char* base = reinterpret_cast<const char*>(src);
            const unsigned step = (unsigned)ld * 4u;
            const unsigned off0 = (unsigned)(kr + g * 8) * step + (unsigned)c0 * 4u;
#pragma unroll
            for (int c = 0; c < NIMG; ++c)
                if (kr + c * KB < K) {
#pragma unroll
                    for (int r = 0; r < 8; ++r)
                        v[c][r] = *reinterpret_cast<const float4*>(base + (off0 + (unsigned)(c * KB + r) * step));
                }
        } else if (vec) {
#pragma unroll
            for (int c = 0; c < NIMG; ++c)
                if (kr + c * KB < K) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[c][r] = fetch4<true>(src, ld, kr + c * KB + g * 8 + r, c0, K, cols);
                }
        } else {
#pragma unroll
            for (int c = 0; c < NIMG; ++c)
                if (kr + c * KB < K) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[c][r] = fetch4<false>(src, ld, kr + c * KB + g * 8 + r, c0, K, cols);
                }
        }
        AIR_STAMP(2);
        if (!(vec && inside && (K % KB) == 0)) {
#pragma unroll
            for (int c = 0; c < NIMG; ++c)
                if (kr + c * KB < K) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) v[c][r] = mask4(v[c][r], kr + c * KB + g * 8 + r, c0, K, cols);
                }
        }
#pragma unroll
        for (int c = 0; c < NIMG; ++c)
            if (kr + c * KB < K) {
                if (bias_thread) {
#pragma unroll
                    for (int r = 0; r < 8; ++r) { csum[0] += v[c][r].x; csum[1] += v[c][r].y; csum[2] += v[c][r].z; csum[3] += v[c][r].w; }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = 4 * q + j;
                    auto e = [&](int r) { const float4& t = v[c][r]; return j == 0 ? t.x : j == 1 ? t.y : j == 2 ? t.z : t.w; };
                    uint4 w;
                    w.x = air_pack_bf16(e(0), e(1)); w.y = air_pack_bf16(e(2), e(3));
                    w.z = air_pack_bf16(e(4), e(5)); w.w = air_pack_bf16(e(6), e(7));
                    *reinterpret_cast<uint4*>(&img[(size_t)c * BT * KB + col * KB + ((g ^ (col & 7)) << 3)]) = w;
                }
            }
        AIR_STAMP(3);
        __syncthreads();
        AIR_STAMP(4);
#pragma unroll
        for (int c = 0; c < NIMG; ++c)
            if (kr + c * KB < K) {
                const unsigned short* ai = Img + (size_t)c * BT * KB;
                const unsigned short* bi = Img + (size_t)(NIMG + c) * BT * KB;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int slot = ks * 4 + (lane >> 4);
                    bf16x8 av[2], bv[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int col = wm + i * 16 + (lane & 15);
                        av[i] = *reinterpret_cast<const bf16x8*>(&ai[col * KB + ((slot ^ (col & 7)) << 3)]);
                    }
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const int col = wn + j * 16 + (lane & 15);
                        bv[j] = *reinterpret_cast<const bf16x8*>(&bi[col * KB + ((slot ^ (col & 7)) << 3)]);
                    }
                    mfma_2x2(acc, av, bv);
                }
            }
    }

    float sq = 0.0f;
    // bias: reduce the 8 k-runs of each column quad; the head units' seven sums go to db[0 .. 6]
    if (bias_block) {
        sum_kruns(csum);
        if (bias_thread && g == 0) sq = head_pack ? store_db(db, csum, 4 * q, 7) : store_db(db, csum, n0 + 4 * q, N);
    }

    // epilogue through LDS
    AIR_STAMP(5);
    __syncthreads();
    acc_to_lds(acc, reinterpret_cast<float*>(Img), wm, wn, lane);       // 64 x LS floats = 20 KB <= 48 KB
    __syncthreads();
    return sq;
}

// ---------------------------------------------------------------------------
// bf16-TWIN tile: both operands are read from the bf16 twins their producers wrote (air_wgrad_t.A16 / dY16).
// K is the slow axis of both, i.e. both are "n-contiguous" for the MFMA: a 64-row image of an operand is
// copied as it lies into a [k][64 columns] LDS image (16- or 8-byte pieces, lane-linear rows of 128 bytes,
// no conversion, no register transpose) and the MFMA fragments -- 8 consecutive k per lane -- come out of
// gfx950's transpose read (read_tr_bf16x8; tools/exp/tr_read.hip; the same scheme as the forward GEMM's
// row-major weights, air_gemm_bf16.hip).  Same bf16 values, same k order per wave as tile_bf16: the tile is
// bit-identical.  The bias gradient still comes from the fp32 dY (column sums before rounding, in tile_bf16's
// order) -- only the tiles that own a column's bias (owns_bias) pay those loads.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool twin_ok(const Prob& pr) {
    // (M % 4 != 0 is fine when the A rows are padded to a multiple of 4: a piece that straddles M stays inside its row, and
    // the output rows it feeds are beyond M -- never stored)
    return pr.A16 && pr.dY16 && !pr.head_pack && rows8(pr.A16, pr.lda) && rows8(pr.dY16, pr.ldb) &&
           ((pr.M & 3) == 0 || pr.lda >= ((pr.M + 3) & ~3)) && (pr.N & 3) == 0;
}

// Bias gradient of a twin tile that owns its column: fp32 column sums of dY[:, n0 .. n0 + 63] in tile_bf16's order -- per
// k-run g the rows g*8 + r of image c, images in order; the xor-tree over g follows.  Run after the MFMAs (the operand
// registers are free), the next image's 8 loads in flight while this one is summed.  (Round 4 tried three images in flight,
// all fetches unconditional: 36.8 -> 31.9 us for a K = 1280 tile that owns a bias, but 9.4 -> 9.8 us at K = 192 and +1.5 us
// on the 50 x 50 step -- not kept.)  Threads 128..255 hold dY's staging role of tile_bf16 (g = k-run of 8 rows, q = column
// quad); returns this thread's share of the squared bias gradient.
__device__ __forceinline__ float bias_tw(const Prob& pr, int n0)
{
    const int tid = threadIdx.x;
    const int N = pr.N, K = pr.K, ldb = pr.ldb;
    const int bg = tid & 7, bq = (tid & 127) >> 3;
    const bool bias_thread = tid >= 128;
    float csum[4] = {0.f, 0.f, 0.f, 0.f};
    if (bias_thread) {
        const bool vec = ((ldb & 3) == 0) && aligned16(pr.dY);
        const int nimg = (K + KB - 1) / KB;
        float4 cur[8], nxt[8];
        auto fetch_img = [&](float4 (&v)[8], int c) __attribute__((always_inline)) {
#pragma unroll
            for (int r = 0; r < 8; ++r)
                v[r] = vec ? fetch4<true>(pr.dY, ldb, c * KB + bg * 8 + r, n0 + 4 * bq, K, N)
                           : fetch4<false>(pr.dY, ldb, c * KB + bg * 8 + r, n0 + 4 * bq, K, N);
        };
        fetch_img(cur, 0);
        for (int c = 0; c < nimg; ++c) {
            if (c + 1 < nimg) fetch_img(nxt, c + 1);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float4 t = mask4(cur[r], c * KB + bg * 8 + r, n0 + 4 * bq, K, N);
                csum[0] += t.x; csum[1] += t.y; csum[2] += t.z; csum[3] += t.w;
            }
#pragma unroll
            for (int r = 0; r < 8; ++r) cur[r] = nxt[r];
        }
    }
    sum_kruns(csum);
    return (bias_thread && bg == 0) ? store_db(pr.db, csum, n0 + 4 * bq, N) : 0.0f;
}

// The same sums with their loads taken off the end of a one-tile workgroup's chain (tile_bf16_tw; one round of images,
// 16-byte rows of dY: bias_early): bias_issue sends image c's eight loads, bias_add adds them in bias_tw's order.  The tile
// issues image 0 behind its operand loads at entry, images 1 and 2 once image 0 is summed, in front of the barrier and the
// MFMAs -- only in the workgroups that own a bias column (block-uniform branches; the registers are never merged with
// other values behind them).  14.1 -> 12.0 us for the launch of the 50 x 50 step: its last workgroups were the owners,
// which fetched their three images one round trip after the other behind the MFMAs.
__device__ __forceinline__ bool bias_early(const Prob& pr) {
    return pr.K <= NIMG_W * KB && (pr.K % KB) == 0 && ((pr.ldb & 3) == 0) && aligned16(pr.dY);
}
// (whole images: every row exists; a column quad at or past N reads quad 0 instead and is masked when added -- one
// per-thread address, the rows at uniform steps)
__device__ __forceinline__ void bias_issue(float4 (&v)[8], const Prob& pr, int n0, int c) {
    const int bg = threadIdx.x & 7, col = n0 + ((threadIdx.x & 127) >> 3) * 4;
    const float* p = pr.dY + ((size_t)(unsigned)(c * KB + bg * 8) * (unsigned)pr.ldb + (unsigned)(col < pr.N ? col : 0));
    const size_t step = (size_t)(unsigned)pr.ldb;
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = *reinterpret_cast<const float4*>(p + r * step);
}
__device__ __forceinline__ void bias_add(float (&csum)[4], const float4 (&v)[8], const Prob& pr, int n0, int c) {
    const int bg = threadIdx.x & 7, bq = (threadIdx.x & 127) >> 3;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float4 t = mask4(v[r], c * KB + bg * 8 + r, n0 + 4 * bq, pr.K, pr.N);
        csum[0] += t.x; csum[1] += t.y; csum[2] += t.z; csum[3] += t.w;
    }
}

// Twin staging of one operand, one round of NIMG_W images: T8 8-byte pieces per thread in registers (two of them = one
// 16-byte piece).  w16 (wave-uniform): 16-byte pieces, piece t = tid + 256 i is row t >> 3, 8 columns from (t & 7) * 8;
// else 8-byte pieces, row t >> 4, 4 columns from (t & 15) * 4.  A piece outside [K x cols] reads element 0 and is
// staged as zeros.  issue_pieces loads, store_pieces puts the registers into the [k][64] image (lane-linear rows).
constexpr int T8 = NIMG_W * KB * 16 / THREADS;
__device__ __forceinline__ void issue_pieces(uint2 (&r)[T8], const char* base, bool w16, int kr, int c0, int K, int cols, int ld) {
    const int tid = threadIdx.x;
    if (w16) {
#pragma unroll
        for (int i = 0; i < T8 / 2; ++i) {
            const int t = tid + THREADS * i, k = kr + (t >> 3), col = c0 + (t & 7) * 8;
            const bool ok = k < K && col < cols;
            const uint4 x = *reinterpret_cast<const uint4*>(base + (ok ? ((unsigned)k * (unsigned)ld + (unsigned)col) * 2u : 0u));
            r[2 * i] = ok ? make_uint2(x.x, x.y) : make_uint2(0u, 0u);
            r[2 * i + 1] = ok ? make_uint2(x.z, x.w) : make_uint2(0u, 0u);
        }
    } else {
#pragma unroll
        for (int i = 0; i < T8; ++i) {
            const int t = tid + THREADS * i, k = kr + (t >> 4), col = c0 + (t & 15) * 4;
            const bool ok = k < K && col < cols;
            const uint2 x = *reinterpret_cast<const uint2*>(base + (ok ? ((unsigned)k * (unsigned)ld + (unsigned)col) * 2u : 0u));
            r[i] = ok ? x : make_uint2(0u, 0u);
        }
    }
}
__device__ __forceinline__ void store_pieces(const uint2 (&r)[T8], unsigned short* img, bool w16) {
    const int tid = threadIdx.x;
    if (w16) {
#pragma unroll
        for (int i = 0; i < T8 / 2; ++i)
            *reinterpret_cast<uint4*>(&img[(tid + THREADS * i) * 8]) = make_uint4(r[2 * i].x, r[2 * i].y, r[2 * i + 1].x, r[2 * i + 1].y);
    } else {
#pragma unroll
        for (int i = 0; i < T8; ++i) *reinterpret_cast<uint2*>(&img[(tid + THREADS * i) * 4]) = r[i];
    }
}

__device__ __forceinline__ float tile_bf16_tw(const Prob& pr, int m0, int n0, unsigned short* Img)
{
    constexpr int NIMG = NIMG_W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int M = pr.M, N = pr.N, K = pr.K, lda = pr.lda, ldb = pr.ldb;
    const char* Ab = reinterpret_cast<const char*>(pr.A16);
    const char* Yb = reinterpret_cast<const char*>(pr.dY16);
    unsigned short* ImgA = Img;                              // [NIMG][64 k][64 m]
    unsigned short* ImgB = Img + NIMG * KB * BT;             // [NIMG][64 k][64 n]
    // 16-byte pieces when rows start 16-byte aligned and are made of whole pieces, else 8-byte pieces (twin_ok)
    const bool a16 = rows16(pr.A16, lda) && (M & 7) == 0;
    const bool b16 = rows16(pr.dY16, ldb) && (N & 7) == 0;
    const bool bias_block = (pr.db != nullptr) && owns_bias(pr, m0, n0);

    f32x4 acc[2][2];
    zero_acc(acc);

    // all operand loads of one round, one wave-uniform branch per operand.  (An interior form of the 16-byte pieces -- one
    // per-thread offset, rows at uniform steps, no compare or select -- was built and measured: 13.96 -> 13.78 us for the
    // launch on its own, 12.01 -> 12.08 beside the early bias sums, i.e. nothing: the launch ends with its slowest
    // workgroup, not with the sum of their instructions.  Removed)
    auto issue_round = [&](uint2 (&ra)[T8], uint2 (&rb)[T8], int kr) __attribute__((always_inline)) {
        issue_pieces(ra, Ab, a16, kr, m0, K, M, lda);
        issue_pieces(rb, Yb, b16, kr, n0, K, N, ldb);
    };
    // ---- MFMAs of one round: fragments through the transpose read
    auto multiply = [&](int kr) __attribute__((always_inline)) {
        const int il = lane & 15;
#pragma unroll
        for (int c = 0; c < NIMG; ++c)
            if (kr + c * KB < K) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int krow = c * KB + ks * 32 + (lane >> 4) * 8 + (il >> 2);
                    const unsigned short* pa = &ImgA[krow * BT + wm + (il & 3) * 4];
                    const unsigned short* pb = &ImgB[krow * BT + wn + (il & 3) * 4];
                    bf16x8 av[2], bv[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) av[i] = read_tr_bf16x8(pa + i * 16, BT);
#pragma unroll
                    for (int j = 0; j < 2; ++j) bv[j] = read_tr_bf16x8(pb + j * 16, BT);
                    mfma_2x2(acc, av, bv);
                }
            }
    };
    float sq = 0.0f;
    const bool early = bias_block && bias_early(pr);          // (bias_early: one round)
    AIR_STAMP(1);
    if (K <= NIMG * KB) {
        // ONE round (every problem of the 50 x 50 step): a path of its own, with no loop around it.  The owner of a bias
        // column (whole images, 16-byte rows: bias_early) sends image 0 of the fp32 dY right behind the operand loads,
        // which are waited for first; sums it as soon as the operands are staged and sends images 1 and 2 into the barrier
        // and the MFMAs (threads 128..255: bias_tw's roles).  One image beside the operand registers, two beside the
        // accumulators: with two at entry the kernel no longer fits its 168 registers (20 bytes of scratch).  The images'
        // registers are live in this path alone.
        const bool bias_wave = early && tid >= 128;
        uint2 ra[T8], rb[T8];
        float4 b0[8], b1[8];
        float csum[4] = {0.f, 0.f, 0.f, 0.f};
        issue_round(ra, rb, 0);
        if (bias_wave) bias_issue(b0, pr, n0, 0);
        AIR_STAMP(2);
        store_pieces(ra, ImgA, a16);
        store_pieces(rb, ImgB, b16);
        if (bias_wave) {
            bias_add(csum, b0, pr, n0, 0);
            if (K > KB) bias_issue(b1, pr, n0, 1);
            if (K > 2 * KB) bias_issue(b0, pr, n0, 2);
        }
        __builtin_amdgcn_sched_barrier(0);                    // (the scheduler would sink the loads below the MFMAs)
        AIR_STAMP(3);
        __syncthreads();
        AIR_STAMP(4);
        multiply(0);
        AIR_STAMP(5);
        if (early) {
            if (bias_wave) {
                if (K > KB) bias_add(csum, b1, pr, n0, 1);
                if (K > 2 * KB) bias_add(csum, b0, pr, n0, 2);
            }
            sum_kruns(csum);
            if (bias_wave && (tid & 7) == 0) sq = store_db(pr.db, csum, n0 + ((tid & 127) >> 3) * 4, N);
        }
    } else {
        // Rounds are software-pipelined: the loads of round r+1 are issued as soon as round r's registers are in LDS, i.e.
        // under its barrier and MFMAs (K > 192: the 128x128 configuration contracts over 256 rows)
        uint2 ra[T8], rb[T8];
        issue_round(ra, rb, 0);
        for (int kr = 0; kr < K; kr += NIMG * KB) {
            if (kr > 0) __syncthreads();
            store_pieces(ra, ImgA, a16);
            store_pieces(rb, ImgB, b16);
            if (kr + NIMG * KB < K) issue_round(ra, rb, kr + NIMG * KB);
            __syncthreads();
            multiply(kr);
        }
    }
    if (bias_block && !early) sq = bias_tw(pr, n0);              // (the one call for every other owner: after the MFMAs)
    __syncthreads();
    acc_to_lds(acc, reinterpret_cast<float*>(Img), wm, wn, lane);
    __syncthreads();
    return sq;
}

// ---------------------------------------------------------------------------
// STRIP workgroup: the 64 x 64 tiles (m0, n0), (m0, n0 + 64), ... of `pr.strip` consecutive column tiles of one
// block-row, for a problem whose output is far larger than its operands -- dWx = X^T . (sum_t dgates) at 128 x 128 is
// 16 384 x 1 024 = 4 096 tiles over K = 256 rows.  One tile per workgroup made every tile fetch its own 32 KB block of the
// image twin (the 16 tiles of a block-row start together on 8 different XCDs) and pay the whole load - stage - multiply -
// store chain (8.9 us a tile with three resident per CU: 48 us for the launch on its own).  Here the A block is fetched ONCE
// and its MFMA fragments stay in registers; the dY tiles stream through one 32 KB image with the next tile's loads in flight
// under this tile's MFMAs, epilogue and stores (3 us a tile); the output tile passes through the same LDS.  Same bf16 values,
// same k order per accumulator, one global-norm partial per TILE at its old index: bit-identical to the per-tile kernel.
// ---------------------------------------------------------------------------
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int STRIP_KMAX = 256;
#ifdef AIR_STAMPS
#ifndef STRIP_STAMP_BLOCK
#define STRIP_STAMP_BLOCK 600
#endif
#define STRIP_STAMP(i) do { if (blockIdx.x == STRIP_STAMP_BLOCK && threadIdx.x == 0) air_stamps_dev[i] = wall_clock64(); } while (0)
#else
#define STRIP_STAMP(i) do { } while (0)
#endif
constexpr int STRIP_LDS = STRIP_KMAX * BT * 2;              // bytes: one [K][64] image (32 KB <= the 48 KB of the one-tile workgroups)
constexpr int STRIP_MAXG = 16;                               // column tiles per strip workgroup, at most
constexpr int STRIP_TAIL = (4 + STRIP_MAXG * 16 + STRIP_MAXG * 4) * 4;   // bytes behind the images: reduction scratch + parked bias
                                                                         // squares + the tiles' squares per wave
template <int NPER,     // 16-byte pieces per thread per operand = K / 32 (a template argument: the operand registers must be
                        // statically indexed -- with a run-time count the compiler kept them in scratch memory and waited for
                        // every load on the spot: 12 us to stage the first images)
          bool A8>      // the A block in 8-byte pieces, masked at M: rows of the A twin are only 8-byte aligned and the last
                        // block-row is ragged (the 50 x 50 canvas: M = lda = 2500)
__device__ __forceinline__ void run_strip_bf16(const Prob& pr, int m0, int n0, unsigned short* Img, float* __restrict__ sq_partials,
                                               int32_t* __restrict__ istate, float* sq_red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int G = pr.strip;
    const unsigned lda = (unsigned)pr.lda, ldb = (unsigned)pr.ldb;
    const char* Ab = reinterpret_cast<const char*>(pr.A16);
    const char* Yb = reinterpret_cast<const char*>(pr.dY16);
    unsigned short* ImgB = Img;                               // [K][64 n] (first the A block, [K][64 m]); then the fp32 output tile
    const bool has_bias = pr.db != nullptr;

    // Bias gradient of the column tiles this block-row owns (owns_bias: at most one of the strip for the big problems),
    // BEFORE the tile loop: the 16 threads that hold a share of its square park it in LDS.
    float* bias_park = sq_red + 4;                            // [strip][16] floats behind the reduction scratch
    float* tile_park = bias_park + STRIP_MAXG * 16;           // [strip][4 waves]: the tiles' squares (park_sq)
    if (has_bias) {
        for (int j = 0; j < G; ++j) {
            if (!owns_bias(pr, m0, n0 + j * BT)) continue;    // block-uniform
            const float b = bias_tw(pr, n0 + j * BT);
            if (tid >= 128 && (tid & 7) == 0) bias_park[j * 16 + ((tid & 127) >> 3)] = b;
        }
        __syncthreads();
    }

    STRIP_STAMP(0);
    // piece t = tid + 256 i: row t >> 3, 8 columns from (t & 7) * 8 -- lane-linear rows of 128 bytes
    const unsigned k0 = (unsigned)(tid >> 3), c8 = (unsigned)(tid & 7) * 8u;
    // (the register images are declared per use, never carried around the tile loop: an array that lives across the
    // loop's back edge stayed in scratch memory, every load waited for on the spot)
    auto issue_b = [&](u32x4 (&rb)[NPER], int nn) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NPER; ++i)
            rb[i] = *reinterpret_cast<const u32x4*>(Yb + ((k0 + 32u * i) * ldb + (unsigned)nn + c8) * 2u);
    };
    auto stage_b = [&](const u32x4 (&rb)[NPER]) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < NPER; ++i)
            *reinterpret_cast<u32x4*>(&ImgB[(tid + THREADS * i) * 8]) = rb[i];
    };
    // The strip is walked from a start that depends on the block-row: the 256 rows of a dY tile lie 2 KB (N * 2 bytes)
    // apart, i.e. in ONE L2 channel, and workgroups that start together stay in step -- all of them on the same tile would
    // queue on that channel (measured: 10 us per tile, the launch twice as slow as one tile per workgroup).
    const int mb = m0 / BT;
    const int rot = (mb + (mb >> 3)) % G;
    auto tile_at = [&](int j) { int t = j + rot; if (t >= G) t -= G; return t; };
    // The A block passes through the image ONCE: each wave keeps the fragments of its 32 columns (all K rows: NPER k-steps
    // x 2 column groups x 4 registers = 64 registers at K = 256) for the whole strip, so a tile reads only dY fragments from
    // LDS (the fragment reads, not the MFMAs, bounded a tile: 128 KB per tile per workgroup at 128 bytes per clock) and the
    // workgroup needs ONE 32 KB image -- three workgroups per CU, like the one-tile workgroups of the same launch.
    const int il = lane & 15;
    bf16x8 av[NPER][2];
    {
        u32x4 rb[NPER];
        if constexpr (!A8) {
            u32x4 ra[NPER];
#pragma unroll
            for (int i = 0; i < NPER; ++i)
                ra[i] = *reinterpret_cast<const u32x4*>(Ab + ((k0 + 32u * i) * lda + (unsigned)m0 + c8) * 2u);
            issue_b(rb, n0 + tile_at(0) * BT);
#pragma unroll
            for (int i = 0; i < NPER; ++i)
                *reinterpret_cast<u32x4*>(&ImgB[(tid + THREADS * i) * 8]) = ra[i];
        } else {
            // piece t = tid + 256 i: row t >> 4, 4 columns from (t & 15) * 4; a piece at or past column M reads element 0
            // and is staged as zeros (M % 4 == 0: pieces are whole)
            u32x2 ra[2 * NPER];
            const unsigned kq = (unsigned)(tid >> 4), c4 = (unsigned)(tid & 15) * 4u;
            const bool okm = m0 + (int)c4 < pr.M;
#pragma unroll
            for (int i = 0; i < 2 * NPER; ++i)
                ra[i] = *reinterpret_cast<const u32x2*>(Ab + (okm ? ((kq + 16u * i) * lda + (unsigned)m0 + c4) * 2u : 0u));
            issue_b(rb, n0 + tile_at(0) * BT);
            const u32x2 zero = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 2 * NPER; ++i)
                *reinterpret_cast<u32x2*>(&ImgB[(tid + THREADS * i) * 4]) = okm ? ra[i] : zero;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < NPER; ++kk) {
            const int krow = kk * 32 + (lane >> 4) * 8 + (il >> 2);
            const unsigned short* pa = &ImgB[krow * BT + wm + (il & 3) * 4];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[kk][i] = read_tr_bf16x8(pa + i * 16, BT);
        }
        __syncthreads();
        stage_b(rb);
    }
    STRIP_STAMP(1);

    const int part0 = pr.first_part + mb * pr.tiles_n + n0 / BT;
    for (int j = 0; j < G; ++j) {
        const int tj = tile_at(j);
        const int nj = n0 + tj * BT;
        __syncthreads();                                      // the images are staged
        STRIP_STAMP(2 + 6 * j);
        // next dY tile: in flight until this tile is stored.  UNCONDITIONAL (the last round re-reads its own tile): behind
        // a branch the loaded registers merge with their old values, and the compiler waits for the loads right here
        u32x4 rb[NPER];
        issue_b(rb, n0 + tile_at(j + 1 < G ? j + 1 : j) * BT);
        __builtin_amdgcn_sched_barrier(0);                    // (the scheduler would sink the loads below the MFMAs)
        f32x4 acc[2][2];
        zero_acc(acc);
#pragma unroll
        for (int kk = 0; kk < NPER; ++kk) {                   // k-steps of 32 rows, in tile_bf16_tw's order
            const int krow = kk * 32 + (lane >> 4) * 8 + (il >> 2);
            const unsigned short* pb = &ImgB[krow * BT + wn + (il & 3) * 4];
            bf16x8 bv[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) bv[jj] = read_tr_bf16x8(pb + jj * 16, BT);
            mfma_2x2(acc, av[kk], bv);
        }
        STRIP_STAMP(3 + 6 * j);
        const float bias_sq = (has_bias && owns_bias(pr, m0, nj) && tid >= 128 && (tid & 7) == 0) ? bias_park[tj * 16 + ((tid & 127) >> 3)] : 0.0f;
        __syncthreads();                                      // every wave is done reading the dY image
        float* Ct = reinterpret_cast<float*>(ImgB);           // 64 x LS floats = 20 KB <= 32 KB
        acc_to_lds(acc, Ct, wm, wn, lane);
        __syncthreads();
        STRIP_STAMP(4 + 6 * j);
        const float sq = store_tile(pr, m0, nj, Ct, bias_sq);
        STRIP_STAMP(5 + 6 * j);
        if (sq_partials) park_sq(sq, tile_park + 4 * tj);   // (no barrier: published behind the loop)
        STRIP_STAMP(6 + 6 * j);
        if (j + 1 < G) {
            __syncthreads();                                  // the output tile has left LDS
            stage_b(rb);
        }
        STRIP_STAMP(7 + 6 * j);
    }
    // the tiles' global-norm partials, one thread per tile: the waves' parked sums in air_block_sum_256's order, at the
    // tile's own index
    if (sq_partials) {
        __syncthreads();
        if (tid < G) publish_parked(tile_park + 4 * tid, sq_partials, istate, part0 + tid);
    }
}
// K = 64 / 128 / 192 / 256 (strip_of) -> NPER, once
template <bool A8>
__device__ __forceinline__ void run_strip_k(const Prob& pr, int m0, int n0, unsigned short* Img, float* __restrict__ sq_partials,
                                            int32_t* __restrict__ istate, float* sq_red)
{
    if (pr.K == 256) run_strip_bf16<8, A8>(pr, m0, n0, Img, sq_partials, istate, sq_red);
    else if (pr.K == 192) run_strip_bf16<6, A8>(pr, m0, n0, Img, sq_partials, istate, sq_red);
    else if (pr.K == 128) run_strip_bf16<4, A8>(pr, m0, n0, Img, sq_partials, istate, sq_red);
    else run_strip_bf16<2, A8>(pr, m0, n0, Img, sq_partials, istate, sq_red);
}

// ---------------------------------------------------------------------------
// BIAS workgroup: db[n0 .. n0 + 63] = column sums of the fp32 dY over all K rows, and its squares as one
// global-norm partial of its own.  For the long contractions (K >= 384: the 128 x 128 configuration's N*B = 1280 rows) the
// column sums were the long pole of the launch when a tile did them on the side -- 128 threads, one 64-row image at a
// time: 21 us on top of the tile's 15.7.  Here they have the launch's FIRST workgroups to themselves (they start at once
// and finish under the tiles), all 256 threads (the two halves take alternate images) and two images in flight per
// thread.  Order of summation (the definition for every operand path and precision of such a problem): thread (h, g, q)
// adds rows 8g .. 8g+7 of its images c = h, h+2, ... in order; xor-tree over g; half 0 + half 1.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void run_bias_wg(const Prob& pr, int n0, int part, float* __restrict__ sq_partials, float* sq_red)
{
    const int tid = threadIdx.x;
    const int N = pr.N, K = pr.K;
    const unsigned ldb = (unsigned)pr.ldb;
    const float* __restrict__ Y = pr.dY;
    const int g = tid & 7, q = (tid >> 3) & 15, h = tid >> 7;
    const int col = n0 + 4 * q;
    const bool vec = ((ldb & 3u) == 0u) && aligned16(Y);
    const int nimg = (K + KB - 1) / KB;
    float csum[4] = {0.f, 0.f, 0.f, 0.f};
    // fetch_img / sum_img mirror fetch4 / mask4 on f32x4 registers: keep them in step.  (Measured, DESIGN.md section 28:
    // written as calls of fetch4 / mask4 on float4, same sums, the stress step was 0.7 % slower.)
    auto fetch_img = [&](f32x4 (&v)[8], int c) __attribute__((always_inline)) {
        if (c >= nimg) c = nimg - 1;                         // (past the end: a valid image again, never summed)
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int row = c * KB + g * 8 + r;
            const bool okr = row < K;
            const unsigned at = (unsigned)row * ldb + (unsigned)col;
            if (vec) v[r] = *reinterpret_cast<const f32x4*>(Y + ((okr && col < N) ? at : 0u));
            else {
                v[r].x = Y[(okr && col < N) ? at : 0u];
                v[r].y = Y[(okr && col + 1 < N) ? at + 1u : 0u];
                v[r].z = Y[(okr && col + 2 < N) ? at + 2u : 0u];
                v[r].w = Y[(okr && col + 3 < N) ? at + 3u : 0u];
            }
        }
    };
    auto sum_img = [&](const f32x4 (&v)[8], int c) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const bool okr = c * KB + g * 8 + r < K;
            csum[0] += (okr && col < N) ? v[r].x : 0.f;
            csum[1] += (okr && col + 1 < N) ? v[r].y : 0.f;
            csum[2] += (okr && col + 2 < N) ? v[r].z : 0.f;
            csum[3] += (okr && col + 3 < N) ? v[r].w : 0.f;
        }
    };
    f32x4 v0[8], v1[8];
    fetch_img(v0, h);
    for (int c = h; c < nimg; c += 4) {
        fetch_img(v1, c + 2);
        __builtin_amdgcn_sched_barrier(0);
        sum_img(v0, c);
        fetch_img(v0, c + 4);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 2 < nimg) sum_img(v1, c + 2);
    }
    sum_kruns(csum);
    float* park = sq_red + 4;                                 // 64 floats: half 1's column sums
    if (h == 1 && g == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) park[4 * q + j] = csum[j];
    }
    __syncthreads();
    float sq = 0.0f;
    if (h == 0 && g == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) csum[j] += park[4 * q + j];
        sq = store_db(pr.db, csum, col, N);
    }
    if (sq_partials) {
        sq = air_block_sum_256(sq, sq_red);
        if (tid == 0) sq_partials[part] = sq;
    }
}

// the launch's first tab.nbias workgroups: bias columns of the long-contraction problems (either precision)
__device__ __forceinline__ void run_bias_block(const Table& tab, int block, float* __restrict__ sq_partials, float* sq_red) {
    int k = 0;                               // the last problem whose bias workgroups start at or before this one
#pragma unroll
    for (int i = 0; i < MAXP; ++i)
        if (i < tab.count && tab.p[i].bias_first >= 0 && block >= tab.p[i].bias_first) k = i;
    const Prob& pb = tab.p[k];
    const int idx = block - pb.bias_first;
    run_bias_wg(pb, idx * BT, pb.bias_part + idx, sq_partials, sq_red);
}

// per-workgroup stamps of the grouped bf16 launch (debug builds with -DAIR_STAMPS only; tools/wgrad_wg_stamps.py):
// [block][4] = start, end, hardware id (XCC_ID << 16 | HW_ID), K * 16 + strip of its problem
#ifdef AIR_STAMPS
static __device__ unsigned long long air_wgrad_wg_stamps[2048 * 4];
#define WG_STAMP(b, i, v) do { if (threadIdx.x == 0 && (b) < 2048) air_wgrad_wg_stamps[(b) * 4 + (i)] = (unsigned long long)(v); } while (0)
#define WG_HWID() ((__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11)) << 16) | __builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11)))
#else
#define WG_STAMP(b, i, v) do { } while (0)
#define WG_HWID() 0
#endif

// One workgroup of the bf16 launch: bias column, strip or tile `block` of the table; Img = 48 KB of LDS (16-byte aligned; a
// strip uses STRIP_LDS of them), sq_red = 4 floats behind it, then the strip's / bias workgroup's parking space.
// sq_partials == NULL: no global-norm partial is published.
__device__ __forceinline__ void run_tile_bf16(const Table& tab, int block, unsigned short* Img, float* __restrict__ sq_partials,
                                              int32_t* __restrict__ istate, float* sq_red)
{
    if (block < tab.nbias) { run_bias_block(tab, block, sq_partials, sq_red); return; }
    int m0, n0;
    const Prob& pr = find_tile(tab, block, m0, n0);
    WG_STAMP(block, 3, pr.K * 16 + pr.strip);
    AIR_STAMP(0);
    if (pr.strip > 0) {
        // the A block in 16-byte pieces: aligned rows and no ragged last block-row
        if (rows16(pr.A16, pr.lda) && (pr.M % BT) == 0) run_strip_k<false>(pr, m0, n0, Img, sq_partials, istate, sq_red);
        else run_strip_k<true>(pr, m0, n0, Img, sq_partials, istate, sq_red);
        return;
    }
    // block-uniform: operands from their bf16 twins where the problem supplies usable ones
    const float bias_sq = twin_ok(pr) ? tile_bf16_tw(pr, m0, n0, Img) : tile_bf16(pr, m0, n0, Img);
    AIR_STAMP(6);
    const float sq = store_tile(pr, m0, n0, reinterpret_cast<const float*>(Img), bias_sq);
    AIR_STAMP(7);
    if (sq_partials) {
        park_sq(sq, sq_red);                                  // (nothing has touched sq_red yet: no barrier in front)
        __syncthreads();
        if (threadIdx.x == 0) publish_parked(sq_red, sq_partials, istate, pr.first_part + (block - pr.first_block));
    }
    AIR_STAMP(8);
}

}  // namespace airw

using namespace airw;

namespace {

__global__ __launch_bounds__(THREADS) void wgrad_grouped_kernel(Table tab, float* __restrict__ sq_partials, int32_t* __restrict__ istate)
{
    __shared__ __attribute__((aligned(16))) float As[2][KC * LS];
    __shared__ __attribute__((aligned(16))) float Bs[2][KC * LS];
    const int block = (int)blockIdx.x;
    __shared__ float sq_red[4 + 64];                            // (+ 64: a bias workgroup parks half of its column sums)
    if (block < tab.nbias) { run_bias_block(tab, block, sq_partials, sq_red); return; }
    int m0, n0;
    const Prob& pr = find_tile(tab, block, m0, n0);
    const float bias_sq = tile_f32<6>(pr, m0, n0, As, Bs);      // K = 192 (3 steps x 64 images) in one round trip
    const float sq = store_tile(pr, m0, n0, &As[0][0], 0.0f) + bias_sq;
    if (sq_partials) publish_sq(sq, sq_partials, istate, pr.first_part + (block - pr.first_block), sq_red);
}


__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 3))) void wgrad_grouped_bf16_kernel(
    Table tab, float* __restrict__ sq_partials, int32_t* __restrict__ istate)
{
    // [operand][image][column 0..63][k 0..63] bf16 = 2 x 3 x 8 KB; reused as the fp32 output tile
    // dynamic: 48 KB of operand images (a strip workgroup uses 32), then STRIP_TAIL bytes: 4 floats for the partial's
    // reduction + the parked bias squares of a strip
    extern __shared__ __attribute__((aligned(16))) unsigned short Img[];
    float* sq_red = reinterpret_cast<float*>(Img + 2 * NIMG_W * BT * KB);
    const int block = (int)blockIdx.x;
    WG_STAMP(block, 0, wall_clock64());
    WG_STAMP(block, 2, WG_HWID());
    run_tile_bf16(tab, block, Img, sq_partials, istate, sq_red);
    WG_STAMP(block, 1, wall_clock64());
}

}  // namespace

AIR_STAMPS_READER(air_debug_stamps_wgrad)
#ifdef AIR_STAMPS
extern "C" int air_debug_stamps_wgrad_wg(unsigned long long* out, int n) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(airw::air_wgrad_wg_stamps), sizeof(unsigned long long) * (n < 2048 * 4 ? n : 2048 * 4));
}
#endif

// ---- host: the table of the launch and the entry points

// Tiles from which a problem counts as BIG (shape alone): it runs in strips when it has twins, and the owners of its bias
// columns are spread over block-rows in every precision.
constexpr long BIG_TILES = 512;
// A problem runs in strips (run_strip_bf16) when its output dwarfs its operands: 4 column tiles per workgroup from 2048
// tiles (dWx at 128 x 128: 4096 tiles over K = 256), 2 from 512 (dWx at 50 x 50: 640 light K = 64 tiles that, one per
// workgroup, pushed the launch past the 768 resident workgroups into a second round).  The A twin in 8-byte rows of whole
// pieces at least, the dY twin in 16-byte rows.
static int strip_of(const air_wgrad_t& g, bool allow) {
    if (!allow || !g.A16 || !g.dY16 || !g.dW || g.head_pack) return 0;
    if (g.K != 64 && g.K != 128 && g.K != 192 && g.K != 256) return 0;
    if (!rows8(g.A16, g.lda) || (g.M & 3) != 0) return 0;
    if (!rows16(g.dY16, g.ldb)) return 0;
    const long tiles = (long)((g.M + BT - 1) / BT) * ((g.N + BT - 1) / BT);
    if (tiles < BIG_TILES) return 0;
    int w = tiles >= 2048 ? 4 : 2;
    if (w > STRIP_MAXG) w = STRIP_MAXG;
    while (w > 1 && (g.N % (BT * w)) != 0) w >>= 1;
    return w > 1 ? w : 0;
}

static int fill_table(const air_wgrad_t* probs, int count, Table& tab, bool allow_null_dw, bool strips = false) {
    if (!probs || count <= 0) return AIR_EINVAL;
    if (count > MAXP) return AIR_ELIMIT;
    tab.count = count;
    // bias columns of the long contractions (K >= 384, shape alone: every precision and operand path agrees) are summed by
    // workgroups of their own, the launch's first (run_bias_wg); their partials follow the tiles'
    int nbias = 0;
    for (int i = 0; i < count; ++i) {
        const air_wgrad_t& g = probs[i];
        if (g.db && !g.head_pack && g.K >= 384 && g.N > 0) nbias += (g.N + BT - 1) / BT;
    }
    tab.nbias = nbias;
    int blocks = nbias, parts = 0, bias_blocks = 0;
    for (int i = 0; i < count; ++i) {
        const air_wgrad_t& g = probs[i];
        if (!g.A || !g.dY || g.M <= 0 || g.N <= 0 || g.K <= 0) return AIR_EINVAL;
        if (!g.dW && (g.head_pack || !allow_null_dw)) return AIR_EINVAL;     // norm-only problems: plain layout, and only with sq_partials
        Prob& p = tab.p[i];
        p.A = g.A; p.dY = g.dY; p.dW = g.dW; p.db = g.db;
        p.A16 = g.A16; p.dY16 = g.dY16;
        p.M = g.M; p.N = g.N; p.K = g.K; p.lda = g.lda; p.ldb = g.ldb; p.ldc = g.ldc;
        p.head_pack = g.head_pack; p.Hs = g.Hs; p.Hh = g.Hh; p.Hz = g.Hz;
        p.tiles_n = (g.N + BT - 1) / BT;
        p.first_block = blocks;
        p.first_part = parts;
        p.bias_first = -1; p.bias_part = -1;
        if (g.db && !g.head_pack && g.K >= 384) { p.bias_first = bias_blocks; p.bias_part = bias_blocks; bias_blocks += p.tiles_n; }
        p.strip = strip_of(g, strips);
        const int tiles_m = (g.M + BT - 1) / BT;
        p.bias_mod = (!g.head_pack && (long)tiles_m * p.tiles_n >= BIG_TILES) ? (tiles_m < 16 ? tiles_m : 16) : 0;
        tab.first[i] = blocks;
        const int tiles = p.tiles_n * ((g.M + BT - 1) / BT);
        parts += tiles;
        blocks += p.strip ? tiles / p.strip : tiles;
    }
    for (int i = count; i < MAXP; ++i) { tab.p[i] = tab.p[0]; tab.first[i] = 0x7fffffff; }
    for (int i = 0; i < count; ++i)
        if (tab.p[i].bias_part >= 0) tab.p[i].bias_part += parts;       // the bias partials follow the tiles'
    tab.total_blocks = parts + nbias;
    tab.launch_blocks = blocks;
    return 0;
}

extern "C" int air_wgrad_num_blocks(const air_wgrad_t* probs, int count) {
    Table tab;
    const int rc = fill_table(probs, count, tab, true);
    return rc ? rc : tab.total_blocks;
}

extern "C" int air_wgrad_num_workgroups(const air_wgrad_t* probs, int count, int precision) {
    if (precision != 0 && precision != 1) return AIR_EINVAL;
    Table tab;
    const int rc = fill_table(probs, count, tab, true, precision == 1);
    return rc ? rc : tab.launch_blocks;
}

extern "C" int air_wgrad_grouped(const air_wgrad_t* probs, int count, int precision,
                                 float* sq_partials, int32_t* istate, void* stream) {
    if (precision != 0 && precision != 1) return AIR_EINVAL;
    Table tab;
    const int rc = fill_table(probs, count, tab, sq_partials != nullptr, precision == 1);
    if (rc) return rc;
    if (precision == 1) {
        static_assert(STRIP_LDS <= 2 * NIMG_W * BT * KB * 2, "a strip image must fit the one-tile workgroups' LDS");
        const size_t lds = sizeof(unsigned short) * 2 * NIMG_W * BT * KB + STRIP_TAIL;
        const int rg = air_grant_lds(reinterpret_cast<const void*>(wgrad_grouped_bf16_kernel), lds);
        if (rg) return rg;
        hipLaunchKernelGGL(wgrad_grouped_bf16_kernel, dim3(tab.launch_blocks), dim3(THREADS), lds, air_stream(stream), tab, sq_partials, istate);
    }
    else hipLaunchKernelGGL(wgrad_grouped_kernel, dim3(tab.launch_blocks), dim3(THREADS), 0, air_stream(stream), tab, sq_partials, istate);
    AIR_CHECK_LAUNCH();
    return 0;
}
