"""The latent clusters restated in numpy float64 (the "latent clusters" section of include/air_hip.h: valid rows, the seeded
start, Lloyd's loop with its tie rule and its sequential sums, the best restart, the table and the counts, the derived
numbers of air.metrics.LatentClusters), and the case table tests/test_latent_kmeans_cases.py (CPU) and
tests/test_gpu_latent_kmeans.py (air_latent_kmeans) share.  No torch, no GPU.

Every operation is a numpy float64 subtract, multiply, add or divide in the header's order: the distance adds e * e dimension
by dimension (a separate multiply and add), the member sums and the inertia are np.add.accumulate over the rows in ascending
order (a strictly sequential sum), the draws are oracle.philox_ref's.  They are correctly rounded IEEE doubles, so the
restatement and the kernel have to give the same BITS.

A case is a dict: x [M, Z] float32, labels [M] int32 or None (the null pointer), k, classes, restarts, max_iters, seed, rows
(None: the null pointer; an int: the value of the device int32).  Rows >= M_eff hold NaN codes and a junk label: they must
never be read."""
import functools
import math

import numpy as np

from oracle import philox_ref

MAX_K, MAX_RESTARTS, MAX_ITERS = 64, 32, 1000
MAX_CLASSES, MAX_Z, MAX_ROWS = 64, 256, 32768                 # the latent probe's
ROWS, VALID, LABELLED, CORRECT, LIVE, BEST, ITERS, CONVERGED, RESTARTS_CONVERGED, COUNTS = range(10)
SALT = 0x4B4D4E53
NAMES = ("accuracy", "ari", "nmi", "inertia", "live_clusters", "scored")
NAN = np.float64(np.nan)                     # the quiet NaN 0x7FF8000000000000
assert NAN.tobytes() == (0x7FF8000000000000).to_bytes(8, "little")
KEYS = ("assignment", "row_d2", "centroids", "restart_inertia", "restart_iters", "counts")


def effective_rows(M, rows):
    return M if rows is None else min(max(int(rows), 0), M)


def workspace_bytes(M, Z, k, R):
    pad8 = lambda n: -(-n // 8) * 8                              # noqa: E731
    return 8 * R * M + 8 * R * k * Z + pad8(4 * R * M) + pad8(4 * M) + pad8(4 * R)


def seq_sum(v):
    """(((+0.0 + v_0) + v_1) + ...): np.add.accumulate is strictly sequential"""
    v = np.asarray(v, np.float64)
    return np.add.accumulate(np.concatenate(([0.0], v)))[-1] if len(v) else np.float64(0.0)


def draws(seed, r, n):
    """word_t of restart r for t < n: word t & 3 of Philox4x32-10, key = seed, counter (r, t >> 2, 0, SALT)"""
    q = -(-n // 4)
    w = philox_ref.philox4x32_10(np.full(q, r), np.arange(q), 0, SALT, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    return w.T.reshape(-1)[:n].astype(np.uint64)


def start_rows(valid_idx, k_eff, seed, r):
    """the k_eff rows restart r starts from: k_eff steps of a Fisher-Yates shuffle of the valid rows"""
    idx, V = list(valid_idx), len(valid_idx)
    for t, word in enumerate(draws(seed, r, k_eff)):
        j = t + int((int(word) * (V - t)) >> 32)
        idx[t], idx[j] = idx[j], idx[t]
    return idx[:k_eff]


def distances(xv, mu):
    """d2 [V, k_eff] of the valid rows xv (float64) and the centroids, z ascending, multiply and add apart"""
    d2 = np.zeros((len(xv), len(mu)), np.float64)
    for z in range(xv.shape[1]):
        e = xv[:, None, z] - mu[None, :, z]
        sq = e * e
        d2 = d2 + sq
    return d2


def lloyd(xv, mu, max_iters):
    """one restart from the centroids mu -> (assignment [V], d2 [V], mu, inertia, iters, converged, the inertia of every
    iteration's assign step)"""
    V, a, trace = len(xv), np.full(len(xv), -1, np.int64), []
    mu = mu.copy()
    for it in range(1, max_iters + 1):
        d2 = distances(xv, mu)
        new = np.argmin(d2, axis=1)                              # the first minimum: a tie goes to the lowest cluster
        best = d2[np.arange(V), new]
        changed = int((new != a).sum())
        a = new
        trace.append(seq_sum(best))
        if changed == 0 or it == max_iters:
            return a, best, mu, trace[-1], it, int(changed == 0), trace
        for c in range(len(mu)):
            members = xv[a == c]
            if len(members):
                mu[c] = np.add.accumulate(np.concatenate((np.zeros((1, xv.shape[1])), members)), axis=0)[-1] / np.float64(len(members))
    raise AssertionError("max_iters < 1")


def kmeans(x, labels, k, classes, restarts, max_iters, seed=0, rows=None, want_trace=False):
    """-> dict(assignment [M] int32, row_d2 [M] float64, centroids [k, Z] float64, restart_inertia [R] float64,
    restart_iters [R] int32, counts int64 [COUNTS + 2 k + k classes])"""
    M, Z = x.shape
    me = effective_rows(M, rows)
    ok = np.isfinite(x[:me]).all(axis=1) if me else np.zeros(0, bool)
    idx = np.nonzero(ok)[0]
    V, ke = len(idx), min(k, len(idx))
    xv = x[idx].astype(np.float64)
    out = dict(assignment=np.full(M, -1, np.int32), row_d2=np.zeros(M, np.float64), centroids=np.full((k, Z), NAN, np.float64),
               restart_inertia=np.full(restarts, NAN, np.float64), restart_iters=np.zeros(restarts, np.int32))
    counts = np.zeros(COUNTS + 2 * k + k * classes, np.int64)
    counts[ROWS], counts[VALID] = me, V
    counts[COUNTS + k:COUNTS + 2 * k] = -1
    out["counts"] = counts
    if V == 0:
        return out
    runs = []
    for r in range(restarts):
        start = start_rows(idx, ke, seed, r)
        runs.append(lloyd(xv, x[start].astype(np.float64), max_iters) + (start,))
        out["restart_inertia"][r], out["restart_iters"][r] = runs[-1][3], runs[-1][4]
    best = 0
    for r in range(1, restarts):
        if out["restart_inertia"][r] < out["restart_inertia"][best]:
            best = r
    a, d2, mu, _, iters, conv, _, _ = runs[best]
    out["assignment"][idx], out["row_d2"][idx], out["centroids"][:ke] = a, d2, mu
    table = np.zeros((k, classes), np.int64)
    if labels is not None:
        lab = labels[idx]
        lab_ok = (lab >= 0) & (lab < classes)
        np.add.at(table, (a[lab_ok], lab[lab_ok]), 1)
    sizes = np.bincount(a, minlength=k)
    counts[LABELLED], counts[CORRECT], counts[LIVE] = table.sum(), table.max(axis=1).sum(), (sizes > 0).sum()
    counts[BEST], counts[ITERS], counts[CONVERGED] = best, iters, conv
    counts[RESTARTS_CONVERGED] = sum(run[5] for run in runs)
    counts[COUNTS:COUNTS + k] = sizes
    counts[COUNTS + k:COUNTS + 2 * k] = np.where(table.max(axis=1) > 0, table.argmax(axis=1), -1)
    counts[COUNTS + 2 * k:] = table.reshape(-1)
    if want_trace:
        out["traces"], out["starts"] = [run[6] for run in runs], [run[7] for run in runs]
    return out


def same_bits(a, b):
    """every output of two results equal as bytes -> the names that differ"""
    return [key for key in KEYS if a[key].dtype != b[key].dtype or a[key].shape != b[key].shape or a[key].tobytes() != b[key].tobytes()]


def parts(counts, k, classes):
    """sizes [k], majority [k], table [k, classes] of a counts array"""
    c = COUNTS
    return counts[c:c + k], counts[c + k:c + 2 * k], counts[c + 2 * k:].reshape(k, classes)


# -------------------------------------------------------------------------------------------------- the derived numbers
def _plogp(p):
    return p * math.log(p) if p > 0 else 0.0


def scores(table):
    """(accuracy, ari, nmi) of a cluster x class table, in Python floats: accuracy = sum_c max_l / n; ari = (I - E) /
    ((A + B) / 2 - E) over the pair counts I = sum C(n_cl, 2), A = sum C(n_c, 2), B = sum C(n_l, 2), E = A B / C(n, 2);
    nmi = 2 I(c; l) / (H(c) + H(l)), natural logarithms.  A zero denominator gives NaN."""
    t = np.asarray(table, np.int64)
    n = int(t.sum())
    nan = float("nan")
    if n == 0:
        return nan, nan, nan
    acc = int(t.max(axis=1).sum()) / n
    pairs = lambda v: float((v * (v - 1) // 2).sum())           # noqa: E731
    I, A, B, N = pairs(t), pairs(t.sum(axis=1)), pairs(t.sum(axis=0)), n * (n - 1) / 2.0
    E = A * B / N if N else nan
    den = (A + B) / 2.0 - E
    ari = (I - E) / den if den == den and den != 0 else nan
    hc = -sum(_plogp(v / n) for v in t.sum(axis=1).tolist())
    hl = -sum(_plogp(v / n) for v in t.sum(axis=0).tolist())
    hcl = -sum(_plogp(v / n) for v in t.reshape(-1).tolist())
    nmi = 2.0 * (hc + hl - hcl) / (hc + hl) if hc + hl != 0 else nan
    return acc, ari, nmi


def entropies(table):
    t = np.asarray(table, np.int64)
    n = int(t.sum())
    return (-sum(_plogp(v / n) for v in t.sum(axis=1).tolist()), -sum(_plogp(v / n) for v in t.sum(axis=0).tolist()))


def derived(result, k, classes):
    """values() of air.metrics.LatentClusters, in NAMES order"""
    counts = result["counts"]
    acc, ari, nmi = scores(parts(counts, k, classes)[2])
    V = int(counts[VALID])
    inertia = float(result["restart_inertia"][counts[BEST]]) / V if V else float("nan")
    return np.asarray([acc, ari, nmi, inertia, counts[LIVE], counts[LABELLED]], np.float64)


def score_allowance(k, classes):
    """|values() - scores()| allowed on ari and nmi: the k classes + k + classes terms p log p of the three entropies are each
    good to a few ulp of a value below 1 / e (the device library's log is within 2 ulp, the product and the quotient p add
    one each: 4), their sums add one rounding per term, and the quotient by H(c) + H(l) > 0.2 magnifies an absolute error by
    at most 2 / 0.2 -- 8 x terms x 2^-52 x 10 covers both scores with a factor of two to spare (ari is exact integer
    arithmetic below 2^53 and five roundings)"""
    return 80.0 * (k * classes + k + classes) * 2.0 ** -52


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(x, labels, k, classes=10, restarts=1, max_iters=50, seed=0, rows=None):
    x = np.ascontiguousarray(x, np.float32)
    me = effective_rows(len(x), rows)
    x[me:] = np.nan                                              # never read
    if labels is not None:
        labels = np.ascontiguousarray(labels, np.int32)
        labels[me:] = 3
    return dict(x=x, labels=labels, k=int(k), classes=int(classes), restarts=int(restarts), max_iters=int(max_iters),
                seed=int(seed), rows=rows)


def _normals(n, seed, call=0):
    """n standard normals of oracle.philox_ref (the Philox equivalent of a RandomState)"""
    return philox_ref.fill_planes(n, 0, seed, call)[0]


def blobs(M, Z, k, classes=10, restarts=1, max_iters=50, seed=0, rows=None, centres=None, sigma=1.0, labelled=True):
    """`centres` (default: classes) Gaussian blobs, row i in blob i % centres, which is its label"""
    centres = classes if centres is None else centres
    mu = 4.0 * _normals(centres * Z, 900 + seed, 1).reshape(centres, Z)
    lab = np.arange(M) % centres
    x = mu[lab] + sigma * _normals(M * Z, 900 + seed, 2).reshape(M, Z)
    return _case(x, lab if labelled else None, k, classes, restarts, max_iters, seed, rows)


THREE_BLOBS_SEED = 21915


def three_blobs():
    """three well separated blobs at M = 65, Z = 3, sigma 0.5: converges in a few iterations, purity 65 / 65, and all eight
    restarts reach the same partition, so their inertias tie to the bit -- BEST is decided by the tie rule.  (Plain random
    starts land in three different blobs about once in four: THREE_BLOBS_SEED is the first seed whose eight restarts all
    do, found by trying the seeds in order.)"""
    centres = np.asarray([[0.0, 0.0, 0.0], [10.0, 0.0, 5.0], [-5.0, 10.0, -5.0]])
    lab = np.arange(65) % 3
    x = centres[lab] + 0.5 * _normals(65 * 3, 31).reshape(65, 3)
    return _case(x, lab, 3, 3, restarts=8, max_iters=50, seed=THREE_BLOBS_SEED)


def one_blob(max_iters):
    x = _normals(257 * 2, 57).reshape(257, 2)
    return _case(x, np.arange(257) % 10, 10, 10, restarts=2, max_iters=max_iters, seed=3)


def duplicates():
    """eight rows holding two distinct values, k = 3: whatever the draws, two of the three start rows coincide or one value
    holds all three; the higher index of a coinciding pair never wins a row and keeps its centroid"""
    x = np.asarray([[1.0, 2.0], [5.0, -1.0]])[[0, 1, 0, 0, 1, 1, 0, 1]]
    return _case(x, [0, 1, 0, 0, 1, 1, 0, 1], 3, 2, restarts=4, max_iters=20, seed=1)


def exact_tie(seed):
    """1-D rows 0, 2, 1: with rows 0 and 1 as the start, row 2 is at distance 1 from both and goes to cluster 0"""
    return _case(np.asarray([[0.0], [2.0], [1.0]]), [0, 1, 0], 2, 2, restarts=1, max_iters=1, seed=seed)


def tie_seed():
    """the first seed whose restart 0 starts from rows (0, 1) in that order"""
    for seed in range(64):
        if start_rows([0, 1, 2], 2, seed, 0) == [0, 1]:
            return seed
    raise AssertionError("no seed below 64 starts from rows 0 and 1")


def _planted(kind):
    c = blobs(37, 5, 4, classes=4, restarts=3, seed=11)
    x, labels = c["x"].copy(), c["labels"].copy()
    rows = None
    if kind == "nan_row":
        x[9, 2] = np.nan
    elif kind == "inf_rows":
        x[9, 4], x[29, 0] = np.inf, -np.inf
    elif kind == "labels_out_of_range":                          # clustered, not scored
        labels[9], labels[10], labels[11] = -1, 4, 1 << 30
    elif kind == "v_below_k":
        x[:, 0] = np.inf
        x[[9, 20], 0] = 0.5, -0.5
    elif kind == "one_valid":
        x[:, 0] = np.inf
        x[9, 0] = 0.5
    elif kind == "all_invalid":
        x[::2, 1], x[1::2, 3] = np.nan, np.inf
    elif kind == "labels_null":
        labels = None
    elif kind == "rows_zero":
        rows = 0
    elif kind == "rows_less":
        rows = 21
    elif kind == "rows_more":
        rows = 500
    elif kind == "rows_negative":
        rows = -3
    return _case(x, labels, 4, 4, restarts=3, max_iters=50, seed=11, rows=rows)


EDGES = ("nan_row", "inf_rows", "labels_out_of_range", "v_below_k", "one_valid", "all_invalid", "labels_null", "rows_zero",
         "rows_less", "rows_more", "rows_negative")
# (M, Z, k, R): every M of {1, 2, 63, 64, 65, 257, 700}, Z of {1, 3, 50}, k of {1, 2, 3, 10}, R of {1, 8}; the last is the
# limits together (the LDS ceiling: 64 x 256 fp64 centroids)
SHAPES = [(1, 1, 1, 1), (2, 3, 2, 1), (63, 50, 10, 1), (64, 3, 3, 8), (65, 50, 2, 8), (257, 3, 10, 8), (700, 50, 10, 1),
          (700, 1, 3, 8), (2, 50, 10, 8), (65, 256, 64, 32)]


def shape_name(s):
    return "m%d_z%d_k%d_r%d" % s


@functools.lru_cache(maxsize=None)
def cases():
    out = {shape_name(s): blobs(s[0], s[1], s[2], restarts=s[3], seed=n, max_iters=30) for n, s in enumerate(SHAPES)}
    out["three_blobs"] = three_blobs()
    out["unconverged"] = one_blob(3)
    out["converged"] = one_blob(100)
    out["duplicates"] = duplicates()
    out["exact_tie"] = exact_tie(tie_seed())
    out.update((kind, _planted(kind)) for kind in EDGES)
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """kmeans() of a case with its traces, computed once and shared: treat it as read-only"""
    c = cases()[name]
    return kmeans(c["x"], c["labels"], c["k"], c["classes"], c["restarts"], c["max_iters"], c["seed"], c["rows"], want_trace=True)
