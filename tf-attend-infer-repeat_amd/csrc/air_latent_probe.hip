// Latent probe: leave-one-out k-nearest-neighbour label accuracy and active units of a set of latent codes -- see the "latent
// probe" section of air_hip.h for the semantics, the order of operations and the summation order.  Four kernels on the
// caller's stream, no synchronisation, no floating-point atomics:
//   probe_valid_kernel    a thread per row: the validity flag of every row (0 for a row >= M_eff, which is not read); the
//                         first workgroup zeroes counts.
//   probe_moments_kernel  a workgroup of AIR_LOC_GROUP threads per dimension: V, then the two fixed-order sums (the adjacent
//                         pairwise tree of air_localization over every group of rows, the group totals in order).
//   probe_pairs_kernel    a workgroup of four waves per (query tile, reference run); lane l of every wave stands for query row
//                         tile * 64 + l, and wave w takes rows [8 w, 8 w + 8) of every reference tile.  The query tile
//                         lies in LDS transposed ([z][lane]: the per-lane reads are conflict-free), the reference rows stream
//                         through LDS in tiles of AIR_PROBE_REF_TILE, widened to fp64 once (every lane reads the same
//                         address: a broadcast), a wave's eight rows in one pass over z.  Each lane keeps its K best (d2, j) pairs sorted in registers: the insertion
//                         is a fully unrolled compare-exchange chain over static indices (a dynamically indexed per-lane
//                         array would live in scratch memory: DESIGN.md section 9).  K = 8 or 16 (two __global__ functions
//                         over one body); the four lists are merged through LDS and the first k pairs go to the workspace.
//   probe_merge_kernel    a thread per row: the partial lists of the runs merged by the same order, the vote, the outputs
//                         and the integer counters.
#include "air_common.h"

namespace {

constexpr int QT = AIR_PROBE_QUERY_TILE;      // queries of a wave
constexpr int RT = AIR_PROBE_REF_TILE;        // reference rows staged at once
constexpr int PAIR_WAVES = 4, PAIR_THREADS = 64 * PAIR_WAVES;
constexpr int JB = AIR_PROBE_PASS_ROWS;       // reference rows a wave takes of a tile: one pass over z
constexpr int MERGE_THREADS = 64;
constexpr int MOM_THREADS = AIR_LOC_GROUP;
constexpr int EMPTY = 0x7fffffff;             // the row of an empty list entry: sorts behind every real pair
static_assert(QT == 64, "a lane per query: the tile is one wave");
static_assert(RT == JB * PAIR_WAVES && MOM_THREADS == 256, "tile and group shapes");

struct ProbeWs { double* pd; int32_t* pj; int32_t* valid; };

__host__ __device__ inline int probe_splits(int M) {
    const int tiles = (M + RT - 1) / RT;
    return tiles < AIR_PROBE_MAX_SPLITS ? tiles : AIR_PROBE_MAX_SPLITS;
}

__device__ __forceinline__ int probe_rows(const air_latent_probe_t& a) {
    if (!a.rows) return a.M;
    const int r = *a.rows;
    return r < 0 ? 0 : (r > a.M ? a.M : r);
}

__device__ __forceinline__ bool probe_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// (d, j) < (D, J) in the order of the header: d2 ascending, then the row ascending
__device__ __forceinline__ bool probe_less(double d, int j, double D, int J) { return d < D || (d == D && j < J); }

template <int K>
struct ProbeList {
    double d[K];
    int j[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int t = 0; t < K; ++t) { d[t] = __builtin_huge_val(); j[t] = EMPTY; }
    }
    // keeps the K smallest pairs sorted: the candidate walks down the list and carries on with what it displaces
    __device__ __forceinline__ void insert(double cd, int cj) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const bool lt = probe_less(cd, cj, d[t], j[t]);
            const double od = d[t];
            const int oj = j[t];
            d[t] = lt ? cd : od;
            j[t] = lt ? cj : oj;
            cd = lt ? od : cd;
            cj = lt ? oj : cj;
        }
    }
};

__global__ __launch_bounds__(256) void probe_valid_kernel(const air_latent_probe_t a, int32_t* __restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0) {
        const int ncounts = AIR_PROBE_COUNTS + a.classes * a.classes;
        for (int c = threadIdx.x; c < ncounts; c += 256) a.counts[c] = 0;
    }
    if (i >= a.M) return;
    int ok = 0;
    if (i < probe_rows(a)) {
        const int lab = a.labels[i];
        ok = lab >= 0 && lab < a.classes;
        const float* x = a.latents + (int64_t)i * a.Z;
        for (int z = 0; z < a.Z; ++z) ok &= probe_finite(x[z]) ? 1 : 0;
    }
    valid[i] = ok;
}

// adjacent pairwise tree over the 256 values of the group, lanes in row order; every thread ends with the total
__device__ __forceinline__ double probe_group_tree(double v, double* red /* [4] */) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_down(v, off, 64);
    __syncthreads();                                             // (the previous group's total has been read)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(MOM_THREADS) void probe_moments_kernel(const air_latent_probe_t a, const int32_t* __restrict__ valid) {
    __shared__ double red[4];
    __shared__ int vcount;
    const int tid = threadIdx.x, z = blockIdx.x, Z = a.Z;
    const int rows = probe_rows(a);
    if (tid == 0) vcount = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < rows; i += MOM_THREADS) mine += valid[i];
    if (mine) atomicAdd(&vcount, mine);                          // an integer: any order, the same sum
    __syncthreads();
    const int V = vcount;
    const int groups = (rows + MOM_THREADS - 1) / MOM_THREADS;
    double S = 0.0;
    for (int g = 0; g < groups; ++g) {
        const int i = g * MOM_THREADS + tid;
        const double v = (i < rows && valid[i]) ? (double)a.latents[(int64_t)i * Z + z] : 0.0;
        S = S + probe_group_tree(v, red);
    }
    const double mean = S / (double)V;
    double Q = 0.0;
    for (int g = 0; g < groups; ++g) {
        const int i = g * MOM_THREADS + tid;
        double v = 0.0;
        if (i < rows && valid[i]) {
            const double e = (double)a.latents[(int64_t)i * Z + z] - mean;
            v = e * e;
        }
        Q = Q + probe_group_tree(v, red);
    }
    if (tid == 0) {
        const double var = Q / (double)V;
        const double nan = __longlong_as_double(0x7FF8000000000000LL);
        a.moments[z] = V ? mean : nan;
        a.moments[Z + z] = V ? var : nan;
        if (V && var > a.au_threshold) atomicAdd(reinterpret_cast<unsigned long long*>(a.counts) + AIR_PROBE_ACTIVE_UNITS, 1ull);
        if (z == 0) { a.counts[AIR_PROBE_ROWS] = rows; a.counts[AIR_PROBE_VALID] = V; }
    }
}

template <int K>
__device__ __forceinline__ void probe_pairs_body(const air_latent_probe_t& a, const ProbeWs& ws, int splits, int tps) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int Z = a.Z, M = a.M, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double* r = reinterpret_cast<double*>(lds_raw);                        // [RT][Z], widened once for all 64 queries
    float* q = reinterpret_cast<float*>(r + (size_t)RT * Z);               // [Z][QT]
    int* rv = reinterpret_cast<int*>(q + (size_t)Z * QT);                  // [RT]
    const int rows = probe_rows(a);
    const int q0 = blockIdx.x * QT, s = blockIdx.y;
    const int i = q0 + lane;
    // the query tile, read as it lies in memory (coalesced) and stored transposed; rows >= M_eff are not read
    const int qrows = min(QT, max(rows - q0, 0));
    const float* qsrc = a.latents + (int64_t)q0 * Z;
    for (int e = tid; e < QT * Z; e += PAIR_THREADS) {
        const int row = e / Z, z = e - row * Z;
        q[z * QT + row] = row < qrows ? qsrc[e] : 0.0f;
    }
    const bool query = i < rows && ws.valid[i] != 0;

    ProbeList<K> best;
    best.clear();
    const int tiles = (M + RT - 1) / RT;
    const int t_end = min((s + 1) * tps, tiles);
    for (int t = s * tps; t < t_end; ++t) {
        const int j0 = t * RT;
        const int rrows = min(RT, max(rows - j0, 0));
        __syncthreads();                                         // the previous tile has been consumed
        const float* rsrc = a.latents + (int64_t)j0 * Z;
        for (int e = tid; e < RT * Z; e += PAIR_THREADS) r[e] = e < rrows * Z ? (double)rsrc[e] : 0.0;
        if (tid < RT) rv[tid] = tid < rrows ? ws.valid[j0 + tid] : 0;
        __syncthreads();
        // wave w takes rows [JB w, JB (w + 1)) of the tile: one pass over z with JB sums in flight
        const int jj = wave * JB;
        bool any = false;
#pragma unroll
        for (int u = 0; u < JB; ++u) any |= rv[jj + u] != 0;
        if (!any) continue;                                      // (uniform in the wave; the barriers are above)
        double acc[JB];
#pragma unroll
        for (int u = 0; u < JB; ++u) acc[u] = 0.0;
        const double* rr = r + (size_t)jj * Z;
#pragma unroll 2
        for (int z = 0; z < Z; ++z) {
            const double xi = (double)q[z * QT + lane];
#pragma unroll
            for (int u = 0; u < JB; ++u) {
                const double e = xi - rr[u * Z + z];
                acc[u] = acc[u] + e * e;
            }
        }
#pragma unroll
        for (int u = 0; u < JB; ++u) {
            const int j = j0 + jj + u;
            // (an invalid reference row may hold anything, a NaN included: its sum is never looked at)
            if (query && rv[jj + u] != 0 && j != i && probe_less(acc[u], j, best.d[K - 1], best.j[K - 1])) best.insert(acc[u], j);
        }
    }
    // the lists of waves 1 .. 3 go through LDS ([wave][entry][lane]: conflict-free) into wave 0's
    __syncthreads();                                             // q and r are free
    double* md = reinterpret_cast<double*>(lds_raw);             // [PAIR_WAVES - 1][K][QT]
    int* mj = reinterpret_cast<int*>(md + (PAIR_WAVES - 1) * K * QT);
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            md[((wave - 1) * K + t) * QT + lane] = best.d[t];
            mj[((wave - 1) * K + t) * QT + lane] = best.j[t];
        }
    }
    __syncthreads();
    if (wave > 0) return;
    for (int w = 0; w < PAIR_WAVES - 1; ++w) {
#pragma unroll
        for (int t = 0; t < K; ++t) {
            const double d = md[(w * K + t) * QT + lane];
            const int j = mj[(w * K + t) * QT + lane];
            if (j != EMPTY && probe_less(d, j, best.d[K - 1], best.j[K - 1])) best.insert(d, j);
        }
    }
    if (i < M) {
        // [run][entry][row]: consecutive lanes store consecutive elements
#pragma unroll
        for (int t = 0; t < K; ++t) {
            if (t < a.k) {
                const int64_t at = ((int64_t)s * a.k + t) * M + i;
                ws.pd[at] = best.d[t];
                ws.pj[at] = best.j[t] == EMPTY ? -1 : best.j[t];
            }
        }
    }
}

__global__ __launch_bounds__(PAIR_THREADS) void probe_pairs_kernel(const air_latent_probe_t a, const ProbeWs ws, int splits, int tps) {
    probe_pairs_body<8>(a, ws, splits, tps);
}
__global__ __launch_bounds__(PAIR_THREADS) void probe_pairs16_kernel(const air_latent_probe_t a, const ProbeWs ws, int splits, int tps) {
    probe_pairs_body<16>(a, ws, splits, tps);
}

template <int K>
__device__ __forceinline__ void probe_merge_body(const air_latent_probe_t& a, const ProbeWs& ws, int splits) {
    const int i = blockIdx.x * MERGE_THREADS + threadIdx.x;
    const int k = a.k, M = a.M;
    const bool row = i < M;
    const int rows = probe_rows(a);
    const int label = (row && i < rows && ws.valid[i]) ? a.labels[i] : -1;     // -1: not a query
    ProbeList<K> best;
    best.clear();
    if (label >= 0) {
        for (int s = 0; s < splits; ++s) {
            for (int t = 0; t < k; ++t) {
                const int64_t at = ((int64_t)s * k + t) * M + i;
                const int j = ws.pj[at];
                if (j < 0) break;                                // a sorted list: the rest is empty too
                const double d = ws.pd[at];
                if (!probe_less(d, j, best.d[K - 1], best.j[K - 1])) break;    // ... and so is everything behind a pair that is too far
                best.insert(d, j);
            }
        }
    }
    // the labels of the kept neighbours (entries t >= k of the merged list lie beyond the k best: dropped here)
    int lab[K];
    int kk = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const bool kept = t < k && best.j[t] != EMPTY;
        lab[t] = kept ? a.labels[best.j[t]] : -1;
        kk += kept ? 1 : 0;
    }
    // the vote without a per-class table: entry t's class has as many votes as entries share its label; the first entry
    // that reaches the largest number is the earliest member of the winning class
    int pred = -1, top = 0;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        int n = 0;
#pragma unroll
        for (int u = 0; u < K; ++u) n += (lab[u] == lab[t]) ? 1 : 0;
        if (lab[t] >= 0 && n > top) { top = n; pred = lab[t]; }
    }
    if (row) {
        if (a.pred) a.pred[i] = pred;
        if (a.neighbours) {
#pragma unroll
            for (int t = 0; t < K; ++t) {
                if (t < k) {
                    const bool kept = best.j[t] != EMPTY;
                    a.neighbours[(int64_t)i * k + t] = kept ? best.j[t] : -1;
                    a.neighbour_d2[(int64_t)i * k + t] = kept ? best.d[t] : 0.0;
                }
            }
        }
    }
    const bool scored = kk > 0;
    const bool correct = scored && pred == label;
    const unsigned long long m_scored = __ballot(scored), m_correct = __ballot(correct);
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(a.counts);
    if ((threadIdx.x & 63) == 0) {                               // integer atomics: any order, the same sums
        if (m_scored) atomicAdd(counts + AIR_PROBE_SCORED, (unsigned long long)__popcll(m_scored));
        if (m_correct) atomicAdd(counts + AIR_PROBE_CORRECT, (unsigned long long)__popcll(m_correct));
    }
    if (scored) atomicAdd(counts + AIR_PROBE_COUNTS + label * a.classes + pred, 1ull);
}

__global__ __launch_bounds__(MERGE_THREADS) void probe_merge_kernel(const air_latent_probe_t a, const ProbeWs ws, int splits) {
    probe_merge_body<8>(a, ws, splits);
}
__global__ __launch_bounds__(MERGE_THREADS) void probe_merge16_kernel(const air_latent_probe_t a, const ProbeWs ws, int splits) {
    probe_merge_body<16>(a, ws, splits);
}

int probe_check_sizes(int M, int Z, int k, int classes) {
    if (M < 1 || Z < 1 || k < 1 || classes < 1) return AIR_EINVAL;
    if (k > AIR_PROBE_MAX_K || classes > AIR_PROBE_MAX_CLASSES || Z > AIR_PROBE_MAX_Z || M > AIR_PROBE_MAX_ROWS) return AIR_ELIMIT;
    return 0;
}

// the workspace: [M, splits, k] fp64 d2 | [M, splits, k] int32 rows (padded to 8 bytes) | [M] int32 validity flags
int64_t probe_list_entries(int M, int k) { return (int64_t)M * probe_splits(M) * k; }
int64_t probe_pad8(int64_t bytes) { return (bytes + 7) / 8 * 8; }

}  // namespace

extern "C" int air_latent_probe_splits(int M) {
    if (M < 1) return AIR_EINVAL;
    if (M > AIR_PROBE_MAX_ROWS) return AIR_ELIMIT;
    return probe_splits(M);
}

extern "C" int64_t air_latent_probe_workspace_bytes(int M, int Z, int k) {
    const int rc = probe_check_sizes(M, Z, k, 1);
    if (rc) return rc;
    const int64_t n = probe_list_entries(M, k);
    return n * 8 + probe_pad8(n * 4) + probe_pad8((int64_t)M * 4);
}

extern "C" int air_latent_probe(const air_latent_probe_t* a, void* workspace, void* stream) {
    if (!a) return AIR_EINVAL;
    if (a->M < 1 || a->Z < 1 || a->k < 1 || a->classes < 1 || !(a->au_threshold >= 0.0)) return AIR_EINVAL;
    const int rc = probe_check_sizes(a->M, a->Z, a->k, a->classes);
    if (rc) return rc;
    if (!a->latents || !a->labels || !a->counts || !a->moments || !workspace) return AIR_EINVAL;
    if (!a->neighbours != !a->neighbour_d2) return AIR_EINVAL;
    if (((uintptr_t)a->moments | (uintptr_t)a->neighbour_d2 | (uintptr_t)workspace) & 7u) return AIR_EALIGN;
    hipStream_t s = air_stream(stream);
    const int M = a->M, Z = a->Z;
    const int splits = probe_splits(M);
    const int tiles = (M + RT - 1) / RT;
    const int tps = (tiles + splits - 1) / splits;
    const int64_t n = probe_list_entries(M, a->k);
    ProbeWs ws;
    ws.pd = static_cast<double*>(workspace);
    ws.pj = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + n * 8);
    ws.valid = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + n * 8 + probe_pad8(n * 4));
    const bool wide = a->k > 8;
    const size_t tile_lds = (size_t)Z * (RT * sizeof(double) + QT * sizeof(float)) + RT * sizeof(int);
    const size_t list_lds = (size_t)(PAIR_WAVES - 1) * (wide ? 16 : 8) * QT * (sizeof(double) + sizeof(int));
    const size_t lds = tile_lds > list_lds ? tile_lds : list_lds;
    const void* fn = wide ? reinterpret_cast<const void*>(probe_pairs16_kernel) : reinterpret_cast<const void*>(probe_pairs_kernel);
    const int grant = air_grant_lds(fn, lds);
    if (grant) return grant;
    const int rowgroups = (M + 255) / 256;
    hipLaunchKernelGGL(probe_valid_kernel, dim3(rowgroups), dim3(256), 0, s, *a, ws.valid);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(probe_moments_kernel, dim3(Z), dim3(MOM_THREADS), 0, s, *a, ws.valid);
    AIR_CHECK_LAUNCH();
    const dim3 grid((M + QT - 1) / QT, splits);
    if (wide) hipLaunchKernelGGL(probe_pairs16_kernel, grid, dim3(PAIR_THREADS), lds, s, *a, ws, splits, tps);
    else hipLaunchKernelGGL(probe_pairs_kernel, grid, dim3(PAIR_THREADS), lds, s, *a, ws, splits, tps);
    AIR_CHECK_LAUNCH();
    const dim3 mgrid((M + MERGE_THREADS - 1) / MERGE_THREADS);
    if (wide) hipLaunchKernelGGL(probe_merge16_kernel, mgrid, dim3(MERGE_THREADS), 0, s, *a, ws, splits);
    else hipLaunchKernelGGL(probe_merge_kernel, mgrid, dim3(MERGE_THREADS), 0, s, *a, ws, splits);
    AIR_CHECK_LAUNCH();
    return 0;
}
