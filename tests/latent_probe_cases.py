"""The latent probe restated in numpy float64 (the "latent probe" section of include/air_hip.h: valid rows, squared
distances, the neighbour order, the vote, the counts, the moments in their ONE summation order, the derived numbers of
air.metrics.LatentProbe), and the case table tests/test_latent_probe_cases.py (CPU) and tests/test_gpu_latent_probe.py
(air_latent_probe) share.  No torch, no GPU.

The restatement is written TWICE: probe() works on whole arrays (every operation a numpy float64 add, subtract, multiply,
divide or comparison, in the header's order along z and along the summation tree), probe_scalar() is a loop over Python
floats that shares nothing with it but the header.  Both are correctly rounded IEEE doubles, so they -- and the kernel --
have to give the same BITS.

A case is a dict: x [M, Z] float32, labels [M] int32, k, classes, au_threshold, rows (None: the null pointer; an int: the
value of the device int32, which may be negative or beyond M) and, for the hand-built ones, planted {name: row}.  Rows
>= M_eff of a case hold NaN codes and a junk label: they must never be read."""
import functools

import numpy as np

MAX_K, MAX_CLASSES, MAX_Z, MAX_ROWS = 16, 64, 256, 32768
QUERY_TILE, REF_TILE, MAX_SPLITS, PASS_ROWS = 64, 32, 8, 8
GROUP = 256                                  # AIR_LOC_GROUP: rows per group of the summation order
ROWS, VALID, SCORED, CORRECT, ACTIVE_UNITS, COUNTS = range(6)
NAMES = ("knn_accuracy", "active_units", "scored", "matched_share")
NAN = np.float64(np.nan)                     # the quiet NaN 0x7FF8000000000000
assert NAN.tobytes() == (0x7FF8000000000000).to_bytes(8, "little")


# ------------------------------------------------------------------------------------------------ the launch's partition
def splits(M):
    return min(MAX_SPLITS, -(-M // REF_TILE))


def tile_of(j):
    return j // REF_TILE


def pass_of(j):
    """the wave of the pairs launch that takes reference row j of its tile"""
    return (j % REF_TILE) // PASS_ROWS


def split_of(j, M):
    tiles = -(-M // REF_TILE)
    return tile_of(j) // -(-tiles // splits(M))


def effective_rows(M, rows):
    return M if rows is None else min(max(int(rows), 0), M)


# -------------------------------------------------------------------------------------------------- on whole arrays
def valid_rows(x, labels, classes):
    return np.isfinite(x).all(axis=1) & (labels >= 0) & (labels < classes)


def tree_sum(v):
    """the ONE order: v (one value per row, 0.0 for an invalid one) in groups of GROUP, each folded by the adjacent pairwise
    tree, the group totals added one by one from +0.0"""
    groups = -(-len(v) // GROUP)
    p = np.zeros(groups * GROUP, np.float64)
    p[:len(v)] = v
    p = p.reshape(groups, GROUP)
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    total = np.float64(0.0)
    for g in range(groups):
        total = total + p[g, 0]
    return total


def probe(x, labels, k, classes, au_threshold=0.01, rows=None):
    """-> dict(pred [M] int32, neighbours [M, k] int32, neighbour_d2 [M, k] float64, counts int64, moments [2 Z] float64)"""
    M, Z = x.shape
    me = effective_rows(M, rows)
    xs, ls = x[:me].astype(np.float64), labels[:me]
    ok = valid_rows(x[:me], ls, classes) if me else np.zeros(0, bool)
    idx = np.nonzero(ok)[0]
    V = len(idx)
    pred = np.full(M, -1, np.int32)
    nb = np.full((M, k), -1, np.int32)
    nd = np.zeros((M, k), np.float64)
    counts = np.zeros(COUNTS + classes * classes, np.int64)
    counts[ROWS], counts[VALID] = me, V
    xv = xs[idx]
    d2 = np.zeros((V, V), np.float64)
    for z in range(Z):
        e = xv[:, None, z] - xv[None, :, z]
        d2 = d2 + e * e
    kk = min(k, V - 1)
    for a, i in enumerate(idx):
        if kk < 1:
            break
        others = np.arange(V) != a
        cand, d = idx[others], d2[a, others]
        order = np.lexsort((cand, d))[:kk]                      # d2 ascending, then the row ascending
        nb[i, :kk], nd[i, :kk] = cand[order], d[order]
        nl = ls[cand[order]]
        votes = np.bincount(nl, minlength=classes)
        pred[i] = nl[np.argmax(votes[nl] == votes.max())]       # the earliest neighbour whose class has the most votes
        counts[SCORED] += 1
        counts[CORRECT] += int(pred[i] == ls[i])
        counts[COUNTS + ls[i] * classes + pred[i]] += 1
    moments = np.full(2 * Z, NAN, np.float64)
    if V:
        for z in range(Z):
            mean = tree_sum(np.where(ok, xs[:, z], 0.0)) / np.float64(V)
            e = xs[:, z] - mean
            var = tree_sum(np.where(ok, e * e, 0.0)) / np.float64(V)
            moments[z], moments[Z + z] = mean, var
            counts[ACTIVE_UNITS] += int(var > au_threshold)
    return dict(pred=pred, neighbours=nb, neighbour_d2=nd, counts=counts, moments=moments)


# ------------------------------------------------------------------------------------------------ on Python floats
def _tree_scalar(values):
    total = 0.0
    for g in range(0, len(values), GROUP):
        v = values[g:g + GROUP] + [0.0] * (GROUP - len(values[g:g + GROUP]))
        while len(v) > 1:
            v = [v[2 * m] + v[2 * m + 1] for m in range(len(v) // 2)]
        total = total + v[0]
    return total


def probe_scalar(x, labels, k, classes, au_threshold=0.01, rows=None):
    M, Z = x.shape
    me = effective_rows(M, rows)
    xs = [[float(v) for v in row] for row in x[:me]]            # float32 -> double, exactly
    ls = [int(v) for v in labels[:me]]
    inf = float("inf")
    ok = [all(v == v and v != inf and v != -inf for v in xs[i]) and 0 <= ls[i] < classes for i in range(me)]
    idx = [i for i in range(me) if ok[i]]
    V = len(idx)
    d2 = {}
    for a, i in enumerate(idx):
        for j in idx[a + 1:]:
            acc = 0.0
            for z in range(Z):
                e = xs[i][z] - xs[j][z]
                acc = acc + e * e
            d2[i, j] = d2[j, i] = acc                           # (e_z only changes sign: the squares are the same)
    pred, nb, nd = [-1] * M, [[-1] * k for _ in range(M)], [[0.0] * k for _ in range(M)]
    counts = [0] * (COUNTS + classes * classes)
    counts[ROWS], counts[VALID] = me, V
    kk = min(k, V - 1)
    for i in idx:
        if kk < 1:
            break
        kept = sorted((d2[i, j], j) for j in idx if j != i)[:kk]
        votes, winner = {}, None
        for _, j in kept:
            votes[ls[j]] = votes.get(ls[j], 0) + 1
        for _, j in kept:                                       # in neighbour order: the first class at the top count
            if votes[ls[j]] == max(votes.values()):
                winner = ls[j]
                break
        pred[i] = winner
        for t, (d, j) in enumerate(kept):
            nb[i][t], nd[i][t] = j, d
        counts[SCORED] += 1
        counts[CORRECT] += int(winner == ls[i])
        counts[COUNTS + ls[i] * classes + winner] += 1
    moments = [float("nan")] * (2 * Z)
    if V:
        for z in range(Z):
            mean = _tree_scalar([xs[i][z] if ok[i] else 0.0 for i in range(me)]) / float(V)
            var = _tree_scalar([(xs[i][z] - mean) * (xs[i][z] - mean) if ok[i] else 0.0 for i in range(me)]) / float(V)
            moments[z], moments[Z + z] = mean, var
            counts[ACTIVE_UNITS] += int(var > au_threshold)
    return dict(pred=np.asarray(pred, np.int32), neighbours=np.asarray(nb, np.int32).reshape(M, k),
                neighbour_d2=np.asarray(nd, np.float64).reshape(M, k), counts=np.asarray(counts, np.int64),
                moments=np.where(np.isnan(moments), NAN, np.asarray(moments, np.float64)))


def same_bits(a, b):
    """every output of two results equal as bytes -> the names that differ"""
    return [key for key in ("pred", "neighbours", "neighbour_d2", "counts", "moments")
            if a[key].dtype != b[key].dtype or a[key].shape != b[key].shape or a[key].tobytes() != b[key].tobytes()]


def derived(counts, matched, present):
    """values() of air.metrics.LatentProbe, in NAMES order: CORRECT / SCORED, ACTIVE_UNITS, SCORED, MATCHED / PRESENT; a
    zero denominator gives NaN"""
    num = np.asarray([counts[CORRECT], counts[ACTIVE_UNITS], counts[SCORED], matched], np.float64)
    den = np.asarray([counts[SCORED], 1, 1, present], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den == 0, NAN, num / den)


def confusion(counts, classes):
    return counts[COUNTS:].reshape(classes, classes)


# ------------------------------------------------------------------------------------------------------------ the cases
def _case(x, labels, k, classes, rows=None, au_threshold=0.01, planted=None):
    x, labels = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(labels, np.int32)
    me = effective_rows(len(x), rows)
    x[me:], labels[me:] = np.nan, 3                              # never read
    return dict(x=x, labels=labels, k=int(k), classes=int(classes), rows=rows, au_threshold=au_threshold,
                planted=planted or {})


def gaussian(M, Z, k=5, classes=10, seed=0, rows=None, spread=1.0):
    """class centres plus noise in the first dimensions, a few dimensions that barely move (inactive units)"""
    rng = np.random.RandomState(1000 * seed + 7 * M + Z)
    labels = rng.randint(0, classes, M)
    centres = rng.randn(classes, Z) * 2.0
    x = centres[labels] + rng.randn(M, Z) * spread
    x[:, Z // 2 + 1:] = 0.25 + 0.01 * rng.randn(M, Z - Z // 2 - 1)      # variance 1e-4: below the 0.01 of Burda et al.
    return _case(x, labels, k, classes, rows)


def half_integer_grid(M=130, Z=3, k=5, classes=10, seed=0):
    """codes on {-1, -0.5, 0, 0.5, 1}^Z: most k-th and (k+1)-th candidates lie at exactly the same distance"""
    rng = np.random.RandomState(seed)
    return _case(rng.randint(-2, 3, (M, Z)) * 0.5, rng.randint(0, classes, M), k, classes)


def duplicates():
    c = gaussian(40, 6, k=5, classes=4, seed=3)
    x, labels = c["x"].copy(), c["labels"].copy()
    x[28:40] = x[:12]                                            # twelve pairs at distance +0.0, eight across a reference tile
    labels[28:34] = labels[:6]
    return _case(x, labels, 5, 4)


def _planted(kind):
    c = gaussian(37, 5, k=3, classes=4, seed=11)
    x, labels, at = c["x"].copy(), c["labels"].copy(), 9
    if kind == "nan_row":
        x[at, 2] = np.nan
    elif kind == "inf_row":
        x[at, 4], x[at + 20, 0] = np.inf, -np.inf
    elif kind == "label_negative":
        labels[at] = -1
    elif kind == "label_too_large":
        labels[at] = 4
    elif kind == "all_invalid":
        x[::2, 1], labels[1::2] = np.nan, 7
    elif kind == "one_valid":
        x[:, 0] = np.inf
        x[at, 0] = 0.5
    return _case(x, labels, 3, 4, planted={kind: at})


VALIDITY = ("nan_row", "inf_row", "label_negative", "label_too_large", "all_invalid", "one_valid")
ROWS_CASES = {"rows_zero": 0, "rows_less": 41, "rows_more": 500, "rows_negative": -3}
# (M, Z, k, classes): M in {1, 2, k, k + 1, 63, 64, 65} and around the reference tile and the full set of splits; Z in {1, 2,
# 50, 51, 256}; k in {1, 5, 16}; classes in {1, 2, 10, 64}
SHAPES = [(1, 50, 5, 10), (2, 50, 5, 10), (5, 50, 5, 10), (6, 50, 5, 10), (63, 50, 5, 10), (64, 50, 5, 10), (65, 50, 5, 10),
          (REF_TILE - 1, 7, 5, 10), (REF_TILE, 7, 5, 10), (REF_TILE + 1, 7, 5, 10), (MAX_SPLITS * REF_TILE + 1, 3, 5, 10),
          (1, 1, 1, 1), (2, 2, 1, 2), (16, 51, 16, 10), (17, 256, 16, 64), (70, 1, 1, 2), (70, 2, 16, 64), (33, 256, 5, 1)]


def shape_name(s):
    return "m%d_z%d_k%d_c%d" % s


@functools.lru_cache(maxsize=None)
def cases():
    out = {shape_name(s): gaussian(*s, seed=n) for n, s in enumerate(SHAPES)}
    out["gaussian"] = gaussian(130, 50, spread=4.0)             # wide enough that some neighbours mislead
    out["ties"] = half_integer_grid()
    out["duplicates"] = duplicates()
    out.update((kind, _planted(kind)) for kind in VALIDITY)
    out.update((name, gaussian(70, 9, seed=5, rows=rows)) for name, rows in ROWS_CASES.items())
    return out


@functools.lru_cache(maxsize=None)
def expected(name):
    """probe() of a case, computed once and shared: treat it as read-only"""
    c = cases()[name]
    return probe(c["x"], c["labels"], c["k"], c["classes"], c["au_threshold"], c["rows"])


def boundary_ties(case):
    """per valid query with more than k candidates: (the k-th and the (k + 1)-th candidate lie at the same d2, their rows)"""
    c = case
    full = probe(c["x"], c["labels"], min(c["k"] + 1, MAX_K + 1), c["classes"], c["au_threshold"], c["rows"])
    k, out = c["k"], {}
    for i in range(len(c["x"])):
        a, b = full["neighbours"][i, k - 1], full["neighbours"][i, k] if full["neighbours"].shape[1] > k else -1
        if a >= 0 and b >= 0:
            out[i] = (full["neighbour_d2"][i, k - 1] == full["neighbour_d2"][i, k], int(a), int(b))
    return out


def shared_top_votes(case, result):
    """the scored rows whose top vote count is reached by more than one class"""
    rows = []
    for i in np.nonzero(result["pred"] >= 0)[0]:
        nb = result["neighbours"][i]
        votes = np.bincount(case["labels"][nb[nb >= 0]], minlength=case["classes"])
        if (votes == votes.max()).sum() > 1:
            rows.append(int(i))
    return rows
