"""Cases, input builders and the float64 restatement of the importance-weighted evaluation bound (include/air_hip.h:
air_importance_logw, air_importance_fold).  The restatement performs the header's operations in the header's order: numpy
element-wise operations over the images (each rounds once, as the device's do with contraction off), plain Python loops
over the steps, the latent dimensions, the samples and the counts, where the order matters.

Synthetic records, not a model, so that the edges are reachable: B = 3 and B = 65 (no multiple of 64; more than one logw
workgroup of 16 images), B = 300 for the fold (two groups of 256), k < B with NaN in rows >= k of every input, T in {1, 2,
16}, Z in {1, 3, 50 with ldz 52, 256}, K in {1, 2, 64}; image 0 stops at step 0 (MASK_PREV_0 = 1, MASK_0 = 0: only its
z_pres term remains), image 1 runs every step, the records of closed steps are NaN; log-weights 800 apart; a degenerate
image (rec_loss = +inf) beside sound ones; an exact tie of the count posterior built from equal log-weights."""
import functools

import numpy as np

MAX_STEPS, MAX_SAMPLES, MAX_Z, GROUP = 16, 64, 256, 256
TERM_REC, TERM_Z_PRES, TERM_SCALE, TERM_SHIFT, TERM_WHAT, TERMS = 0, 1, 2, 3, 4, 5
IMAGES, SCORED, DEGENERATE, MAP_CORRECT, SPLIT, COUNTS = 0, 1, 2, 3, 4, 5
BOUND, ELBO, ESS, ENTROPY, SUMS = 0, 1, 2, 3, 4
NAMES = ("nll_bound", "sample_loss", "gap", "ess_share", "count_accuracy", "count_entropy", "count_split")
# the slots of include/air_hip.h the restatement reads (tests/test_importance_abi.py holds them against the binding)
ATT_S, ATT_X, ATT_Y, ATT_KL_Z, ATT_MASK_PREV, ATT_MASK, ATT_STRIDE, OUT_STRIDE = 0, 1, 2, 6, 10, 11, 16, 8
OUT_SCALE_LV, OUT_SHIFT_LV_X, OUT_SHIFT_LV_Y = 1, 4, 5
DYN_SCALE, DYN_SHIFT, DYN_VAE, DYN_COUNT = (5, 6, 13), (7, 8, 14), (9, 10, 15), 16        # (PM, PV, PLV) of each prior
EPS = 2.0 ** -52

# (B, k, T, Z, ldz, K)
LOGW_SHAPES = ((3, 3, 1, 1, 1, 1), (65, 60, 2, 3, 3, 2), (65, 65, 16, 50, 52, 64), (3, 2, 3, 256, 256, 2), (20, 17, 3, 50, 52, 3))
PRIORS = dict(scale=(-1.0, 0.05), shift=(0.0, 1.0), vae=(0.125, 0.75))


def shape_name(s):
    return "b%d_k%d_t%d_z%d_ld%d_s%d" % tuple(s)


def fold_bound(K, T):
    """what the fp64 values of the fold may differ by, relative to max(1, |ref|): the device's exp and log are held to 3 ulp
    (the OpenCL limit) and a sum has at most K + T terms"""
    return 8.0 * (K + T + 2) * EPS


# ------------------------------------------------------------------------------------------------------------- log-weights
def logw_inputs(shape, seed=0, rec_inf=()):
    """the buffers of one pass as float32 / int32 arrays.  rec_inf: images whose rec_loss is +inf"""
    B, k, T, Z, ldz, K = shape
    rng, f, nan = np.random.RandomState(1000 * seed + B + 7 * T + Z), np.float32, np.float32("nan")
    n = rng.randint(0, T + 1, size=B)
    n[0] = 0
    if B > 1:
        n[1] = T
    att = rng.standard_normal((T, B, ATT_STRIDE)).astype(f)
    att[:, :, ATT_S] = rng.uniform(0.05, 0.95, (T, B))
    att[:, :, ATT_X:ATT_Y + 1] = rng.uniform(-0.95, 0.95, (T, B, 2))
    out7 = (0.5 * rng.standard_normal((T, B, OUT_STRIDE))).astype(f)
    ml = (0.7 * rng.standard_normal((T, B, 2 * Z))).astype(f)
    z = rng.standard_normal((T, B, ldz)).astype(f)
    z[:, :, Z:] = nan                                            # the pad columns of a row are never read
    eps_scale, eps_shift = rng.standard_normal((T, B)).astype(f), rng.standard_normal((T, B, 2)).astype(f)
    eps_z = rng.standard_normal((T, B, Z)).astype(f)
    for t in range(T):
        on, prev = t < n, t <= n                                 # MASK_t, MASK_PREV_t (= MASK_{t-1}; 1 at t = 0)
        att[t, ~prev] = nan                                      # a step the image never reached: the whole record
        for buf in (out7, ml, z, eps_scale, eps_shift, eps_z):
            buf[t, ~on] = nan                                    # a closed step: what it sampled
        att[t, ~on, ATT_S:ATT_Y + 1] = nan
        att[t, :, ATT_MASK], att[t, :, ATT_MASK_PREV] = on, prev
    rec_loss = rng.uniform(50.0, 400.0, B).astype(f)
    rec_loss[list(rec_inf)] = np.inf
    run_digits = n.astype(np.int32)
    for buf in (att, out7, ml, z, eps_scale, eps_shift, eps_z):
        buf[:, k:] = nan                                         # rows >= k of every input
    rec_loss[k:], run_digits[k:] = nan, -77
    dyn = np.full(DYN_COUNT, nan, f)
    for slots, (pm, pv) in ((DYN_SCALE, PRIORS["scale"]), (DYN_SHIFT, PRIORS["shift"]), (DYN_VAE, PRIORS["vae"])):
        dyn[list(slots)] = pm, pv, np.log(np.float32(pv))
    return dict(att=att, out7=out7, ml=ml, z=z, eps_scale=eps_scale, eps_shift=eps_shift, eps_z=eps_z, rec_loss=rec_loss,
                run_digits=run_digits, dyn=dyn, shape=tuple(shape), steps=n)


def lr_gauss(z, eps, lv, pm, pv, plv):
    """log q(z) - log p(z) at the sample: the header's lr, operation by operation"""
    return 0.5 * ((((z - pm) * (z - pm)) / pv + plv) - eps * eps - lv)


def logw_reference(inp):
    """(logw [k], digits [k], terms [k, 5]) of one pass: the header's arithmetic on widened inputs"""
    B, k, T, Z, ldz, K = inp["shape"]
    d = lambda a: np.asarray(a, dtype=np.float64)                # noqa: E731
    att, out7, dyn = inp["att"], inp["out7"], inp["dyn"]
    prior = lambda slots: tuple(np.float64(dyn[s]) for s in slots)                      # noqa: E731
    loss = d(inp["rec_loss"][:k])
    terms = np.zeros((k, TERMS))
    terms[:, TERM_REC] = loss
    with np.errstate(invalid="ignore"):
        for t in range(T):
            rec = att[t, :k]
            scale = lr_gauss(d(rec[:, ATT_S]), d(inp["eps_scale"][t, :k]), d(out7[t, :k, OUT_SCALE_LV]), *prior(DYN_SCALE))
            shift = lr_gauss(d(rec[:, ATT_X]), d(inp["eps_shift"][t, :k, 0]), d(out7[t, :k, OUT_SHIFT_LV_X]), *prior(DYN_SHIFT)) + \
                lr_gauss(d(rec[:, ATT_Y]), d(inp["eps_shift"][t, :k, 1]), d(out7[t, :k, OUT_SHIFT_LV_Y]), *prior(DYN_SHIFT))
            what = np.zeros(k)
            for j in range(Z):
                what = what + lr_gauss(d(inp["z"][t, :k, j]), d(inp["eps_z"][t, :k, j]), d(inp["ml"][t, :k, Z + j]), *prior(DYN_VAE))
            on, prev = rec[:, ATT_MASK] != 0, rec[:, ATT_MASK_PREV] != 0
            a = np.where(prev, d(rec[:, ATT_KL_Z]), 0.0)
            b = np.where(on, (scale + shift) + what, 0.0)
            loss = loss + (a + b)
            terms[:, TERM_Z_PRES] = terms[:, TERM_Z_PRES] + a
            for col, v in ((TERM_SCALE, scale), (TERM_SHIFT, shift), (TERM_WHAT, what)):
                terms[:, col] = terms[:, col] + np.where(on, v, 0.0)
    return -loss, inp["run_digits"][:k].copy(), terms


# -------------------------------------------------------------------------------------------------------------------- fold
def group_sum(values, k):
    """the ONE order of the sums: groups of GROUP images (+0.0 beyond k) folded by the adjacent pairwise tree, the group
    totals added in group order from +0.0"""
    groups = -(-k // GROUP)
    v = np.zeros(groups * GROUP)
    v[:k] = values
    total = np.float64(0.0)
    for g in range(groups):
        w = v[g * GROUP:(g + 1) * GROUP]
        while len(w) > 1:
            w = w[0::2] + w[1::2]
        total = total + w[0]
    return total


def fold_reference(case, counts_in=None, sums_in=None):
    """counts, sums and the per-image values of one air_importance_fold call over `case`"""
    T, k, K = case["T"], case["k"], case["K"]
    logw, digits, targets = case["logw"], case["digits"], case["targets"]
    counts = np.zeros(COUNTS + (T + 1) * (T + 1), np.int64) if counts_in is None else counts_in.copy()
    per = {key: np.zeros(k) for key in ("bound", "elbo", "ess", "entropy")}
    out = dict(bound=np.full(k, np.nan), ess=np.full(k, np.nan), map=np.full(k, -1, np.int32), split=np.zeros(k, bool),
               degenerate=np.zeros(k, bool), W=np.zeros((k, T + 1)), elbo=np.full(k, np.nan))
    Kd = np.float64(K)
    for i in range(k):
        l = [np.float64(logw[s, i]) for s in range(K)]
        m = l[0]
        for s in range(1, K):
            if l[s] > m or l[s] != l[s]:
                m = l[s]
        counts[IMAGES] += 1
        if not np.isfinite(m):
            counts[DEGENERATE] += 1
            out["degenerate"][i] = True
            continue
        dg = [min(max(int(digits[s, i]), 0), T) for s in range(K)]
        S = S2 = L = np.float64(0.0)
        e = [np.exp(l[s] - m) for s in range(K)]
        for s in range(K):
            S = S + e[s]
            S2 = S2 + e[s] * e[s]
            L = L + l[s]
        bound, ess = m + np.log(S / Kd), (S * S) / S2
        best, cmap, ent = np.float64(0.0), 0, np.float64(0.0)
        for c in range(T + 1):
            W = np.float64(0.0)
            for s in range(K):
                if dg[s] == c:
                    W = W + e[s]
            out["W"][i, c] = W
            if c == 0 or W > best:
                best, cmap = W, c
            if W != 0.0:
                p = W / S
                ent = ent + p * np.log(p)
        split = any(v != dg[0] for v in dg)
        per["bound"][i], per["elbo"][i], per["ess"][i], per["entropy"][i] = bound, L / Kd, ess, -ent
        out["bound"][i], out["ess"][i], out["map"][i], out["split"][i], out["elbo"][i] = bound, ess, cmap, split, L / Kd
        counts[SCORED] += 1
        counts[SPLIT] += int(split)
        if targets is not None:
            g = min(max(int(targets[i]), 0), T)
            counts[MAP_CORRECT] += int(g == cmap)
            counts[COUNTS + g * (T + 1) + cmap] += 1
    sums = np.zeros(SUMS) if sums_in is None else sums_in.copy()
    for slot, key in ((BOUND, "bound"), (ELBO, "elbo"), (ESS, "ess"), (ENTROPY, "entropy")):
        sums[slot] = sums[slot] + group_sum(per[key], k)
    out.update(counts=counts, sums=sums, entropy=per["entropy"])
    return out


def values_of(counts, sums, K, has_targets=True):
    """the seven names() from the accumulators, as ImportanceBound.values() derives them"""
    sc = float(counts[SCORED])
    if sc == 0:
        return [float("nan")] * len(NAMES)
    return [-sums[BOUND] / sc, -sums[ELBO] / sc, (sums[BOUND] - sums[ELBO]) / sc, sums[ESS] / (sc * K),
            counts[MAP_CORRECT] / sc if has_targets else float("nan"), sums[ENTROPY] / sc, counts[SPLIT] / sc]


def _tables(B, k, T, K, seed, targets=True):
    rng = np.random.RandomState(seed)
    spread = rng.choice([0.1, 1.0, 30.0], size=B)                # near-equal weights, a few effective samples, one sample
    logw = -(200.0 + 40.0 * rng.standard_normal(B)) + spread * rng.standard_normal((K, B))
    digits = rng.randint(0, T + 1, size=(K, B)).astype(np.int32)
    digits[:, ::3] = digits[0, ::3]                              # a third of the images agree on the count
    logw[:, k:], digits[:, k:] = np.nan, -77
    return dict(logw=logw, digits=digits, targets=rng.randint(0, T + 1, size=k).astype(np.int32) if targets else None,
                T=T, B=B, k=k, K=K)


@functools.lru_cache(maxsize=None)
def degenerate_passes():
    """K = 2 passes of the (3, 3, 2, 3, 3, 2) shape in which image 2 has rec_loss = +inf"""
    return tuple(logw_inputs((3, 3, 2, 3, 3, 2), seed=40 + s, rec_inf=(2,)) for s in range(2))


@functools.lru_cache(maxsize=None)
def fold_cases():
    cases = {"b3_t1_s1": _tables(3, 3, 1, 1, 1), "b65_t2_s2": _tables(65, 60, 2, 2, 2), "b65_t16_s64": _tables(65, 65, 16, 64, 3),
             "b300_t3_s16": _tables(300, 290, 3, 16, 4), "no_targets": _tables(65, 60, 2, 2, 2, targets=False)}
    c = cases["b65_t2_s2"]                                       # counts beyond [0, T] are clamped
    c["digits"][0, 5], c["digits"][1, 6], c["targets"][7] = 2 + 3, -2, 2 + 9
    cases["underflow"] = dict(logw=np.array([[-100.0, -100.0, -900.0], [-900.0, -100.5, -100.0]]),
                              digits=np.array([[1, 2, 0], [2, 2, 1]], np.int32), targets=np.array([1, 2, 2], np.int32),
                              T=2, B=3, k=3, K=2)
    cases["tie"] = dict(logw=np.array([[-310.25, -77.5, -120.0]] * 4),
                        digits=np.array([[1, 2, 1], [1, 0, 1], [2, 0, 1], [2, 2, 1]], np.int32),
                        targets=np.array([2, 0, 1], np.int32), T=2, B=3, k=3, K=4)
    rows = [logw_reference(p) for p in degenerate_passes()]
    cases["degenerate"] = dict(logw=np.stack([r[0] for r in rows]), digits=np.stack([r[1] for r in rows]).astype(np.int32),
                               targets=np.array([0, 2, 1], np.int32), T=2, B=3, k=3, K=2)
    return cases


TIED = {"tie": (0, 1)}                                           # case -> the images whose count posterior ties exactly
DEGENERATE_IMAGES = {"degenerate": (2,)}


@functools.lru_cache(maxsize=None)
def expected_fold(name):
    return fold_reference(fold_cases()[name])


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def close(got, want, K, T):
    """the largest gap of two fp64 arrays relative to max(1, |want|), and whether it is within fold_bound(K, T); a NaN must
    meet a NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return float("inf"), False
    ok = ~np.isnan(want)
    gap = float(np.max(np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok])))) if ok.any() else 0.0
    return gap, gap <= fold_bound(K, T)
