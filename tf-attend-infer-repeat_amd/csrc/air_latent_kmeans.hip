// Latent clusters: exact k-means (Lloyd's loop with restarts) over a set of latent codes and the cluster x class table of
// the best restart -- see the "latent clusters" section of air_hip.h for the semantics, the order of every operation and
// the summation orders.  Three kernels on the caller's stream, no synchronisation, no floating-point atomics, no grid-wide
// wait:
//   kmeans_valid_kernel    a thread per row: the validity flag of every row (0 for a row >= M_eff, which is not read).
//   kmeans_restart_kernel  a workgroup per restart, its whole loop inside the kernel.  The centroids live in LDS (fp64,
//                          [k][Z]: up to 128 KiB) and are updated IN PLACE: the assign step is over when the update begins, and
//                          every (cluster, dimension) sum is owned by ONE thread that zeroes it, walks the rows in ascending
//                          order and divides -- the stated order, no atomics and no second [k][Z] block.  A thread owns
//                          dimension z of the clusters c = g (mod NG), NG = min(k_eff, threads / Z); when NG == k_eff that is
//                          one cluster, and the sum stays in a register.  Assign: a thread per row, KM_CB clusters in one pass
//                          over z (every lane reads the same centroid element: an LDS broadcast).  `changed` is a
//                          workgroup-wide OR through a flag in LDS: every barrier is reached by all threads or by none, every
//                          trip count is bounded by a range-checked argument.  The restart's assignment, d2 and centroids go
//                          to the workspace, its inertia (one thread, rows in order) and iterations to the outputs.
//   kmeans_pick_kernel     one workgroup: the first minimum of the inertias, the winner copied out, table / sizes in LDS by
//                          integer atomics, then majority and the counts.
#include "air_common.h"
#include "air_philox.h"

namespace {

constexpr int KM_THREADS = 1024;              // of a restart's workgroup: Z <= 256 leaves NG >= 4 cluster groups
constexpr int KM_CB = 8;                      // clusters an assign pass over z carries
constexpr int KM_WALK = 32;                   // rows a sequential walk loads at once (the adds stay in row order)
constexpr int PICK_THREADS = 256;
constexpr uint32_t KM_SALT = 0x4B4D4E53u;     // "KMNS": c3 of the seeding draws
static_assert(AIR_PROBE_MAX_Z <= KM_THREADS, "a thread per dimension");

struct KmWs { double* d2; double* cent; int32_t* a; int32_t* valid; int32_t* conv; };

// THE layout of the restart kernel's dynamic LDS (byte offsets): the launch sizes it and the kernel carves it from here
struct KmLds { size_t mu, n, seed, pos, val, misc, total; };
__host__ __device__ inline KmLds kmeans_lds(int k, int Z) {
    KmLds l;
    l.mu = 0;                                           // double [k][Z]  the centroids
    l.n = (size_t)k * Z * sizeof(double);               // int [k]        members
    l.seed = l.n + (size_t)k * sizeof(int);             // int [k]        the seeding draw: a rank among the valid rows, then its row
    l.pos = l.seed + (size_t)k * sizeof(int);           // int [2 k]      the live swaps of the partial shuffle: position ...
    l.val = l.pos + (size_t)2 * k * sizeof(int);        // int [2 k]      ... and what lies there
    l.misc = l.val + (size_t)2 * k * sizeof(int);       // int [4]        V, the `changed` flag
    l.total = l.misc + 4 * sizeof(int);
    return l;
}

__device__ __forceinline__ int km_rows(const air_latent_kmeans_t& a) {
    if (!a.rows) return a.M;
    const int r = *a.rows;
    return r < 0 ? 0 : (r > a.M ? a.M : r);
}

__device__ __forceinline__ bool km_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void kmeans_valid_kernel(const air_latent_kmeans_t a, int32_t* __restrict__ valid) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.M) return;
    int ok = 0;
    if (i < km_rows(a)) {
        ok = 1;
        const float* x = a.latents + (int64_t)i * a.Z;
        for (int z = 0; z < a.Z; ++z) ok &= km_finite(x[z]) ? 1 : 0;
    }
    valid[i] = ok;
}

__global__ __launch_bounds__(KM_THREADS) void kmeans_restart_kernel(const air_latent_kmeans_t a, const KmWs ws) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const KmLds L = kmeans_lds(a.k, a.Z);
    double* mu = reinterpret_cast<double*>(lds_raw + L.mu);
    int* n = reinterpret_cast<int*>(lds_raw + L.n);
    int* seed = reinterpret_cast<int*>(lds_raw + L.seed);
    int* pos = reinterpret_cast<int*>(lds_raw + L.pos);
    int* val = reinterpret_cast<int*>(lds_raw + L.val);
    int* misc = reinterpret_cast<int*>(lds_raw + L.misc);
    const int tid = threadIdx.x, r = blockIdx.x, M = a.M, Z = a.Z;
    const int rows = km_rows(a);
    int32_t* asg = ws.a + (int64_t)r * M;
    double* d2 = ws.d2 + (int64_t)r * M;
    double* cent = ws.cent + (int64_t)r * a.k * Z;
    const double nan = __longlong_as_double(0x7FF8000000000000LL);

    if (tid == 0) { misc[0] = 0; misc[1] = 0; }
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < rows; i += KM_THREADS) mine += ws.valid[i];
    if (mine) atomicAdd(&misc[0], mine);                         // an integer: any order, the same sum
    for (int i = tid; i < M; i += KM_THREADS) { asg[i] = -1; d2[i] = 0.0; }
    __syncthreads();
    const int V = misc[0];
    const int ke = a.k < V ? a.k : V;
    if (V == 0) {                                                // (uniform: every thread leaves, no barrier behind)
        for (int e = tid; e < a.k * Z; e += KM_THREADS) cent[e] = nan;
        if (tid == 0) { a.restart_inertia[r] = nan; a.restart_iters[r] = 0; ws.conv[r] = 0; }
        return;
    }

    // the start: k_eff steps of a Fisher-Yates shuffle of the valid rows' ranks; only the touched positions are held
    if (tid == 0) {
        AirDraws<KM_SALT> draws((uint32_t)r, 0u, a.seed);
        int live = 0;
        for (int t = 0; t < ke; ++t) {
            const int j = draws.range(t, V - t);
            int vt = t, vj = j, st = -1, sj = -1;
            for (int u = 0; u < live; ++u) {
                if (pos[u] == t) { vt = val[u]; st = u; }
                if (pos[u] == j) { vj = val[u]; sj = u; }
            }
            if (st < 0) { st = live++; pos[st] = t; }
            val[st] = vj;
            if (j != t) {
                if (sj < 0) { sj = live++; pos[sj] = j; }
                val[sj] = vt;
            }
            seed[t] = vj;                                        // idx[t]: later swaps touch positions > t only
        }
    }
    __syncthreads();
    if (tid < ke) {                                              // the rank among the valid rows -> the row
        const int want = seed[tid];
        int cnt = 0, row = -1;
        for (int i0 = 0; i0 < rows && row < 0; i0 += KM_WALK) {  // KM_WALK independent loads, then the count in order
            int v[KM_WALK];
#pragma unroll
            for (int u = 0; u < KM_WALK; ++u) v[u] = i0 + u < rows ? ws.valid[i0 + u] : 0;
#pragma unroll
            for (int u = 0; u < KM_WALK; ++u) {
                if (v[u]) {
                    if (cnt == want && row < 0) row = i0 + u;
                    ++cnt;
                }
            }
        }
        seed[tid] = row < 0 ? 0 : row;                           // (want < V: always found)
    }
    __syncthreads();
    for (int e = tid; e < ke * Z; e += KM_THREADS) {
        const int c = e / Z, z = e - c * Z;
        mu[e] = (double)a.latents[(int64_t)seed[c] * Z + z];
    }
    __syncthreads();

    const int ng_most = KM_THREADS / Z;
    const int NG = ke < ng_most ? ke : ng_most;                  // >= 1: Z <= KM_THREADS and k_eff >= 1
    const int g = tid / Z, z_own = tid - g * Z;
    int it = 1, conv = 0;
    for (;; ++it) {                                              // it <= max_iters <= AIR_KMEANS_MAX_ITERS: left below
        int changed = 0;
        for (int i = tid; i < rows; i += KM_THREADS) {
            if (!ws.valid[i]) continue;
            const float* x = a.latents + (int64_t)i * Z;
            double bd = 0.0;
            int bc = -1;
            for (int c0 = 0; c0 < ke; c0 += KM_CB) {
                double acc[KM_CB];
                const double* m[KM_CB];
#pragma unroll
                for (int u = 0; u < KM_CB; ++u) {
                    acc[u] = 0.0;
                    const int c = c0 + u < ke ? c0 + u : ke - 1;   // (beyond k_eff: a valid address, the sum is dropped)
                    m[u] = mu + (size_t)c * Z;
                }
#pragma unroll 4
                for (int z = 0; z < Z; ++z) {                    // (unrolled: four loads of the row in flight)
                    const double xi = (double)x[z];
#pragma unroll
                    for (int u = 0; u < KM_CB; ++u) {
                        const double e = xi - m[u][z];
                        acc[u] = acc[u] + e * e;
                    }
                }
#pragma unroll
                for (int u = 0; u < KM_CB; ++u) {
                    const int c = c0 + u;
                    if (c < ke && (bc < 0 || acc[u] < bd)) { bd = acc[u]; bc = c; }     // a tie keeps the lower cluster
                }
            }
            changed |= (bc != asg[i]) ? 1 : 0;
            asg[i] = bc;
            d2[i] = bd;
        }
        // the workgroup-wide OR through the dynamic block (__syncthreads_or brings 256 bytes of static LDS, which the
        // 160 KiB grant has no room for: DESIGN.md section 26.5); misc[1] is 0 here, and zeroed again behind two barriers
        if (changed) misc[1] = 1;
        __syncthreads();                                         // (also: asg and d2 are visible to the workgroup)
        const int any = misc[1];
        __syncthreads();
        if (tid == 0) misc[1] = 0;                               // (the next write lies behind the barriers of the update)
        if (!any) { conv = 1; break; }
        if (it >= a.max_iters) break;
        for (int c = tid; c < ke; c += KM_THREADS) n[c] = 0;
        __syncthreads();
        for (int i = tid; i < rows; i += KM_THREADS)
            if (ws.valid[i]) atomicAdd(&n[asg[i]], 1);
        __syncthreads();
        if (g < NG) {
            const float* col = a.latents + z_own;
            if (NG == ke) {                                      // one cluster of this dimension: the sum in a register
                if (n[g] > 0) {
                    double S = 0.0;
                    for (int i0 = 0; i0 < rows; i0 += KM_WALK) {  // KM_WALK independent loads, then the adds in row order
                        int cc[KM_WALK];
                        float xv[KM_WALK];
#pragma unroll
                        for (int u = 0; u < KM_WALK; ++u) {
                            const int i = i0 + u < rows ? i0 + u : rows - 1;     // (the tail: a row in use, dropped by its -1)
                            cc[u] = i0 + u < rows ? asg[i] : -1;
                            xv[u] = col[(int64_t)i * Z];
                        }
#pragma unroll
                        for (int u = 0; u < KM_WALK; ++u) S = cc[u] == g ? S + (double)xv[u] : S;   // a SELECT: another
                    }                                                                               // row's NaN goes nowhere
                    mu[(size_t)g * Z + z_own] = S / (double)n[g];
                }
            } else {
                for (int c = g; c < ke; c += NG)
                    if (n[c] > 0) mu[(size_t)c * Z + z_own] = 0.0;
                for (int i0 = 0; i0 < rows; i0 += KM_WALK) {
                    int cc[KM_WALK];
                    float xv[KM_WALK];
#pragma unroll
                    for (int u = 0; u < KM_WALK; ++u) {
                        const int i = i0 + u < rows ? i0 + u : rows - 1;
                        cc[u] = i0 + u < rows ? asg[i] : -1;
                        xv[u] = col[(int64_t)i * Z];
                    }
#pragma unroll
                    for (int u = 0; u < KM_WALK; ++u) {
                        const int c = cc[u];
                        if (c >= 0 && c % NG == g) {
                            double* s = mu + (size_t)c * Z + z_own;
                            *s = *s + (double)xv[u];
                        }
                    }
                }
                for (int c = g; c < ke; c += NG)
                    if (n[c] > 0) mu[(size_t)c * Z + z_own] = mu[(size_t)c * Z + z_own] / (double)n[c];
            }
        }
        __syncthreads();
    }
    for (int e = tid; e < a.k * Z; e += KM_THREADS) cent[e] = e < ke * Z ? mu[e] : nan;
    if (tid == 0) {
        double s = 0.0;
        for (int i0 = 0; i0 < rows; i0 += KM_WALK) {
            int v[KM_WALK];
            double d[KM_WALK];
#pragma unroll
            for (int u = 0; u < KM_WALK; ++u) {
                const int i = i0 + u < rows ? i0 + u : rows - 1;
                v[u] = i0 + u < rows ? ws.valid[i] : 0;
                d[u] = d2[i];
            }
#pragma unroll
            for (int u = 0; u < KM_WALK; ++u) s = v[u] ? s + d[u] : s;
        }
        a.restart_inertia[r] = s;
        a.restart_iters[r] = it;
        ws.conv[r] = conv;
    }
}

__global__ __launch_bounds__(PICK_THREADS) void kmeans_pick_kernel(const air_latent_kmeans_t a, const KmWs ws) {
    __shared__ int table[AIR_KMEANS_MAX_K * AIR_PROBE_MAX_CLASSES];
    __shared__ int sizes[AIR_KMEANS_MAX_K];
    __shared__ int sh[6];                                        // V, best, converged restarts, labelled, correct, live
    const int tid = threadIdx.x, M = a.M, Z = a.Z, k = a.k, classes = a.classes, R = a.restarts;
    const int rows = km_rows(a);
    for (int e = tid; e < k * classes; e += PICK_THREADS) table[e] = 0;
    if (tid < k) sizes[tid] = 0;
    if (tid < 6) sh[tid] = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < rows; i += PICK_THREADS) mine += ws.valid[i];
    if (mine) atomicAdd(&sh[0], mine);
    if (tid == 0) {
        int b = 0, nconv = ws.conv[0];
        for (int r = 1; r < R; ++r) {
            if (a.restart_inertia[r] < a.restart_inertia[b]) b = r;      // the first minimum (NaN, V == 0: restart 0)
            nconv += ws.conv[r];
        }
        sh[1] = b;
        sh[2] = nconv;
    }
    __syncthreads();
    const int V = sh[0], b = sh[1];
    const int32_t* asg = ws.a + (int64_t)b * M;
    const double* d2 = ws.d2 + (int64_t)b * M;
    for (int i = tid; i < M; i += PICK_THREADS) {
        const bool ok = i < rows && ws.valid[i] != 0;
        const int c = ok ? asg[i] : -1;
        a.assignment[i] = c;
        if (a.row_d2) a.row_d2[i] = ok ? d2[i] : 0.0;
        if (ok) {
            atomicAdd(&sizes[c], 1);
            if (a.labels) {
                const int lab = a.labels[i];
                if (lab >= 0 && lab < classes) atomicAdd(&table[c * classes + lab], 1);
            }
        }
    }
    const double* cent = ws.cent + (int64_t)b * k * Z;
    for (int e = tid; e < k * Z; e += PICK_THREADS) a.centroids[e] = cent[e];
    __syncthreads();
    int64_t* sizes_out = a.counts + AIR_KMEANS_COUNTS;
    int64_t* majority = sizes_out + k;
    int64_t* table_out = majority + k;
    if (tid < k) {
        int top = 0, arg = -1, sum = 0;
        for (int l = 0; l < classes; ++l) {
            const int v = table[tid * classes + l];
            sum += v;
            if (v > top) { top = v; arg = l; }                   // the first maximum; no labelled member: -1
        }
        sizes_out[tid] = sizes[tid];
        majority[tid] = arg;
        if (sum) atomicAdd(&sh[3], sum);
        if (top) atomicAdd(&sh[4], top);
        if (sizes[tid] > 0) atomicAdd(&sh[5], 1);
    }
    for (int e = tid; e < k * classes; e += PICK_THREADS) table_out[e] = table[e];
    __syncthreads();
    if (tid == 0) {
        a.counts[AIR_KMEANS_ROWS] = rows;
        a.counts[AIR_KMEANS_VALID] = V;
        a.counts[AIR_KMEANS_LABELLED] = sh[3];
        a.counts[AIR_KMEANS_CORRECT] = sh[4];
        a.counts[AIR_KMEANS_LIVE] = sh[5];
        a.counts[AIR_KMEANS_BEST] = b;
        a.counts[AIR_KMEANS_ITERS] = a.restart_iters[b];
        a.counts[AIR_KMEANS_CONVERGED] = ws.conv[b];
        a.counts[AIR_KMEANS_RESTARTS_CONVERGED] = sh[2];
    }
}

int kmeans_check_sizes(int M, int Z, int k, int restarts) {
    if (M < 1 || Z < 1 || k < 1 || restarts < 1) return AIR_EINVAL;
    if (k > AIR_KMEANS_MAX_K || restarts > AIR_KMEANS_MAX_RESTARTS || Z > AIR_PROBE_MAX_Z || M > AIR_PROBE_MAX_ROWS) return AIR_ELIMIT;
    return 0;
}

int64_t kmeans_pad8(int64_t bytes) { return (bytes + 7) / 8 * 8; }

}  // namespace

// the workspace: [R, M] fp64 d2 | [R, k, Z] fp64 centroids | [R, M] int32 assignments | [M] int32 validity flags | [R] int32
// converged flags, each int32 block padded to 8 bytes
extern "C" int64_t air_latent_kmeans_workspace_bytes(int M, int Z, int k, int restarts) {
    const int rc = kmeans_check_sizes(M, Z, k, restarts);
    if (rc) return rc;
    const int64_t R = restarts;
    return 8 * R * M + 8 * R * k * Z + kmeans_pad8(4 * R * M) + kmeans_pad8(4 * (int64_t)M) + kmeans_pad8(4 * R);
}

extern "C" int air_latent_kmeans(const air_latent_kmeans_t* a, void* workspace, void* stream) {
    if (!a) return AIR_EINVAL;
    if (a->M < 1 || a->Z < 1 || a->k < 1 || a->classes < 1 || a->restarts < 1 || a->max_iters < 1) return AIR_EINVAL;
    const int rc = kmeans_check_sizes(a->M, a->Z, a->k, a->restarts);
    if (rc) return rc;
    if (a->classes > AIR_PROBE_MAX_CLASSES || a->max_iters > AIR_KMEANS_MAX_ITERS) return AIR_ELIMIT;
    if (!a->latents || !a->assignment || !a->centroids || !a->restart_inertia || !a->restart_iters || !a->counts || !workspace)
        return AIR_EINVAL;
    if (((uintptr_t)a->row_d2 | (uintptr_t)a->centroids | (uintptr_t)a->restart_inertia | (uintptr_t)workspace) & 7u) return AIR_EALIGN;
    hipStream_t s = air_stream(stream);
    const int64_t M = a->M, R = a->restarts;
    char* w = static_cast<char*>(workspace);
    KmWs ws;
    ws.d2 = reinterpret_cast<double*>(w);
    w += 8 * R * M;
    ws.cent = reinterpret_cast<double*>(w);
    w += 8 * R * a->k * a->Z;
    ws.a = reinterpret_cast<int32_t*>(w);
    w += kmeans_pad8(4 * R * M);
    ws.valid = reinterpret_cast<int32_t*>(w);
    w += kmeans_pad8(4 * M);
    ws.conv = reinterpret_cast<int32_t*>(w);
    const size_t lds = kmeans_lds(a->k, a->Z).total;
    const int grant = air_grant_lds(reinterpret_cast<const void*>(kmeans_restart_kernel), lds);
    if (grant) return grant;
    hipLaunchKernelGGL(kmeans_valid_kernel, dim3((a->M + 255) / 256), dim3(256), 0, s, *a, ws.valid);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(kmeans_restart_kernel, dim3(a->restarts), dim3(KM_THREADS), lds, s, *a, ws);
    AIR_CHECK_LAUNCH();
    hipLaunchKernelGGL(kmeans_pick_kernel, dim3(1), dim3(PICK_THREADS), 0, s, *a, ws);
    AIR_CHECK_LAUNCH();
    return 0;
}
