"""The CNN front-end (csrc/air_cnn.hip; include/air_hip.h, "stand-alone CNN front-end") restated in numpy float64 with its
routing rules written out, the restatement of the kernels' LDS layout, and the case tables that
tests/test_cnn_edge_cases.py (CPU: every condition on the inputs) and tests/test_gpu_cnn_edges.py (the C ABI on guarded
buffers) share.  No GPU, no library call.

THE BLOCK.  NHWC, kernels [5, 5, Cin, F]:
  pre1 = conv5x5_SAME(image, k1) + b1;  r1 = pre1 where pre1 > 0 else 0;  pool1, arg1 = pool(r1)      [S  -> S1 = S  // 2]
  pre2 = conv5x5_SAME(pool1, k2) + b2;  r2 likewise;                      pool2, arg2 = pool(r2)      [S1 -> S2 = S1 // 2]
  pre3 = conv5x5_SAME(pool2, k3) + b3;  out = r3 flattened (y, x, channel)
  pool: 2x2 / stride 2 VALID (an odd last row and column are dropped); the value is the maximum of the window, the code
  2 dy + dx names the FIRST maximum in row-major window order: a later element replaces the best one only when it is
  strictly greater (`first_max` below says so itself and does not lean on a library's tie behaviour).
  Gradients of sum(d_out * out): the ReLU of a layer passes a gradient only where its output is > 0 (an exact zero does
  not pass), read as out > 0, pool2 > 0 and pool1 > 0 (pool(relu(x)) = relu(pool(x)): the pooled value of the window is
  its argmax site's ReLU output); the pool passes it to the site its code names, every other site of the window gets 0.

TWO KINDS OF INPUTS.
  exact-integer (`exact_case`): images in {0..3}, kernel taps from {-1, 0, 0, 1}, biases in {-1, 0, 1}, d_out from
    {-1, 0, 0, 1}.  Every product and every partial sum of every chain is an integer, so ANY accumulation order in fp32
    gives the float64 value exactly as long as the sum of |term| of each chain stays below 2^24 (`bounds`, computed with
    absolute-value convolutions from the reference alone, summed over the batch for the variable gradients).  Exact zeros
    and ties are abundant, so these cases pin `>` against `>=` in the pool and in the three masks (`bites` counts the sites
    at which the other rule would change a gradient).
  real-valued (`real_case`): the recipe of tests/test_gpu_cnn.py (its _variables, uniform [0, 1) images, normal d_out) with
    that file's precondition -- ReLU margin and pool margin >= 1e-5 on the float64 reference -- at the first seed from 1
    upward that meets it.  At the last canvases (~ 60 000 pre-activations an image) no seed meets it: `real_forward_case`
    carries the forward only, which is continuous across a flipped branch."""
import functools

import numpy as np

f32 = np.float32
NAMES = ["cnn/conv%d/%s" % (i, kind) for i in (1, 2, 3) for kind in ("kernel", "bias")]
MARGIN = 1e-5                       # tests/test_gpu_cnn.py's precondition
EXACT_LIMIT = float(2 ** 24)
LDS_LIMIT = 160 * 1024              # AIR_LDS_LIMIT of csrc/air_common.h, bytes
FWD_NT, BWD_NT = 256, 512           # threads of cnn_fwd_kernel / cnn_bwd_kernel
SQ_GROUP = 256                      # gradient elements per workgroup of cnn_reduce_sq_kernel


# ---------------------------------------------------------------------------------------------- the LDS layout, restated
def r2(v):
    return (v + 1) & ~1


def r4(v):
    return (v + 3) & ~3


def cnn_lds(S, F):
    """cnn_lds() of csrc/air_cnn.hip (struct CnnLds, the function under it) in floats, plus which side each of its two
    max() choices took: r1_is (g3h | p2h against the haloed image), r4_is (compact d_pre1 + codes against the haloed pool1)"""
    L = {}
    S1 = S >> 1
    S2 = S1 >> 1
    FP = r4(F)
    IP, P1, P2 = r2(S + 4), r2(S1 + 4), r2(S2 + 4)
    img_n, pl1, pl2 = r4(IP * (S + 4)), P1 * (S1 + 4), P2 * (S2 + 4)
    wn = r4(25 * F * FP)
    L.update(S1=S1, S2=S2, FP=FP, IP=IP, P1=P1, P2=P2, img_n=img_n, pl1=pl1, pl2=pl2)
    L["f_w1"] = 0
    L["f_w2"] = r4(25 * FP)
    L["f_w3"] = L["f_w2"] + wn
    L["f_bias"] = L["f_w3"] + wn
    L["f_img"] = L["f_bias"] + r4(3 * FP)
    L["f_p1"] = L["f_img"] + img_n
    L["f_p2"] = L["f_p1"] + r4(F * pl1)
    L["f_total"] = L["f_p2"] + r4(F * pl2)
    L["b_w3"], L["b_w2"], L["b_k1"] = 0, wn, 2 * wn
    L["b_r1"] = L["b_k1"] + r4(25 * FP)
    pair, image = 2 * r4(F * pl2), img_n
    L["r1_is"] = "g3h|p2h" if pair > image else "image"
    L["b_r2"] = L["b_r1"] + max(pair, image)
    L["b_r4"] = L["b_r2"] + r4(F * pl1)
    d1 = r4(F * S1 * S1)
    compact, haloed = d1 + r4((F * S1 * S1 + 3) // 4), r4(F * pl1)
    L["r4_is"] = "compact+codes" if compact > haloed else "haloed"
    L["b_code"] = L["b_r4"] + d1
    L["b_total"] = L["b_r4"] + max(compact, haloed)
    L["bytes"] = 4 * max(L["f_total"], L["b_total"])
    return L


def num_partials(F):
    """cnn_num_partials: floats of one image's dk1 | db1 | dk2 | db2 | dk3 | db3"""
    return 25 * F + 50 * F * F + 3 * F


def num_sq_partials(F):
    return (num_partials(F) + SQ_GROUP - 1) // SQ_GROUP


def served(S, F):
    """cnn_check: 0, or the library's error code for the size"""
    if S < 4 or F < 1:
        return -1
    if F > 8 or S > 128:
        return -2
    return -2 if cnn_lds(S, F)["bytes"] > LDS_LIMIT else 0


LAST_CANVAS = {8: 77, 7: 83, 6: 89, 5: 97, 4: 107, 3: 118, 2: 128, 1: 128}   # tests/test_cnn_abi.py's table


# ---------------------------------------------------------------------------------------------------- float64 reference
def conv(h, k, b):
    """5x5 SAME + bias: h [B, n, n, Cin], k [5, 5, Cin, F] -> [B, n, n, F]"""
    n = h.shape[1]
    hp = np.pad(h, ((0, 0), (2, 2), (2, 2), (0, 0)))
    out = np.zeros(h.shape[:3] + (k.shape[3],)) + b
    for ky in range(5):
        for kx in range(5):
            out += hp[:, ky:ky + n, kx:kx + n, :] @ k[ky, kx]
    return out


def conv_data_grad(g, k):
    """d input of conv: g [B, n, n, F] -> [B, n, n, Cin];  d_in[y, x] = sum over taps of g[y - ky + 2, x - kx + 2] . k[ky, kx]"""
    n = g.shape[1]
    gp = np.pad(g, ((0, 0), (2, 2), (2, 2), (0, 0)))
    out = np.zeros(g.shape[:3] + (k.shape[2],))
    for ky in range(5):
        for kx in range(5):
            out += gp[:, 4 - ky:4 - ky + n, 4 - kx:4 - kx + n, :] @ k[ky, kx].T
    return out


def conv_kernel_grad(h, g):
    """per image: dk [B, 5, 5, Cin, F] and db [B, F] from the layer's input h and its pre-activation gradient g"""
    n = h.shape[1]
    hp = np.pad(h, ((0, 0), (2, 2), (2, 2), (0, 0)))
    dk = np.zeros((h.shape[0], 5, 5, h.shape[3], g.shape[3]))
    for ky in range(5):
        for kx in range(5):
            dk[:, ky, kx] = np.einsum("byxc,byxf->bcf", hp[:, ky:ky + n, kx:kx + n, :], g)
    return dk, g.sum(axis=(1, 2))


def relu(pre):
    return np.where(pre > 0.0, pre, 0.0)


def windows(r):
    """[B, n, n, F] -> [B, m, m, F, 4], element 2 dy + dx of each 2x2 window (m = n // 2: an odd last row / column is dropped)"""
    B, n, _, F = r.shape
    m = n // 2
    return r[:, :2 * m, :2 * m, :].reshape(B, m, 2, m, 2, F).transpose(0, 1, 3, 5, 2, 4).reshape(B, m, m, F, 4)


def first_max(r):
    """pooled value and code of the FIRST maximum: element j replaces the best one only when strictly greater"""
    win = windows(r)
    best = win[..., 0].copy()
    code = np.zeros(best.shape, np.uint8)
    for j in (1, 2, 3):
        better = win[..., j] > best
        best = np.where(better, win[..., j], best)
        code = np.where(better, np.uint8(j), code)
    return best, code


def unpool(g, code, n):
    """[B, m, m, F] at the sites the codes name of a zero [B, n, n, F]"""
    m = g.shape[1]
    out = np.zeros((g.shape[0], n, n, g.shape[3]))
    for j in range(4):
        out[:, (j >> 1):2 * m:2, (j & 1):2 * m:2, :] = np.where(code == j, g, 0.0)
    return out


def _margins(pres, rs):
    relu_margin = min(float(np.abs(p).min()) for p in pres)
    pool_margin = float("inf")
    for r in rs:
        top = np.sort(windows(r), axis=-1)
        live = top[..., 3] > 0
        if live.any():
            pool_margin = min(pool_margin, float((top[..., 3] - top[..., 2])[live].min()))
    return relu_margin, pool_margin


def reference(P, images, d_out=None):
    """float64.  P: {name: array}; images [B, S * S]; d_out [B, S2 * S2 * F] or None (forward only).
    -> out, pool1, pool2 (float64), arg1, arg2 (uint8), relu_margin, pool_margin and, with d_out: d_images, the six gradients
    under their names, `partials` [B, num_partials(F)] (one image's dk1 | db1 | dk2 | db2 | dk3 | db3 per row), `bounds`
    {chain: largest sum of |term|}, `bites` {rule: sites at which the other rule would move a gradient}"""
    k1, b1, k2, b2, k3, b3 = [np.asarray(P[n], np.float64) for n in NAMES]
    B = images.shape[0]
    S = int(round(np.sqrt(images.shape[1])))
    F = k1.shape[3]
    x = np.asarray(images, np.float64).reshape(B, S, S, 1)
    pre1 = conv(x, k1, b1); r1 = relu(pre1); p1, a1 = first_max(r1)
    pre2 = conv(p1, k2, b2); r2_ = relu(pre2); p2, a2 = first_max(r2_)
    pre3 = conv(p2, k3, b3); out = relu(pre3)
    S1, S2 = p1.shape[1], p2.shape[1]
    ref = dict(out=out.reshape(B, -1), pool1=p1, pool2=p2, arg1=a1, arg2=a2)
    ref["relu_margin"], ref["pool_margin"] = _margins((pre1, pre2, pre3), (r1, r2_))
    ref["zeros"] = int((pre1 == 0).sum() + (pre2 == 0).sum() + (pre3 == 0).sum())
    if d_out is not None:
        go = np.asarray(d_out, np.float64).reshape(B, S2, S2, F)
        g3 = np.where(out > 0.0, go, 0.0)
        dk3, db3 = conv_kernel_grad(p2, g3)
        dp2 = conv_data_grad(g3, k3)
        g2 = unpool(np.where(p2 > 0.0, dp2, 0.0), a2, S1)
        dk2, db2 = conv_kernel_grad(p1, g2)
        dp1 = conv_data_grad(g2, k2)
        g1 = unpool(np.where(p1 > 0.0, dp1, 0.0), a1, S)
        dk1, db1 = conv_kernel_grad(x, g1)
        ref["d_images"] = conv_data_grad(g1, k1).reshape(B, S * S)
        per_image = [dk1, db1, dk2, db2, dk3, db3]
        for n, g in zip(NAMES, per_image):
            ref[n] = g.sum(axis=0)
        ref["partials"] = np.concatenate([g.reshape(B, -1) for g in per_image], axis=1)
        # the largest sum of |term| of every chain the kernels run (any order of it), the batch sums included
        A = np.abs
        ref["bounds"] = {
            "pre1": conv(A(x), A(k1), A(b1)).max(), "pre2": conv(p1, A(k2), A(b2)).max(), "pre3": conv(p2, A(k3), A(b3)).max(),
            "d_pool2": conv_data_grad(A(g3), A(k3)).max(), "d_pool1": conv_data_grad(A(g2), A(k2)).max(),
            "d_images": conv_data_grad(A(g1), A(k1)).max(),
            "dk3": conv_kernel_grad(p2, A(g3))[0].sum(axis=0).max(), "db3": A(g3).sum(axis=(0, 1, 2)).max(),
            "dk2": conv_kernel_grad(p1, A(g2))[0].sum(axis=0).max(), "db2": A(g2).sum(axis=(0, 1, 2)).max(),
            "dk1": conv_kernel_grad(A(x), A(g1))[0].sum(axis=0).max(), "db1": A(g1).sum(axis=(0, 1, 2)).max()}
        # where `>=` in place of `>` would change what the backward computes: a gradient arriving at an exact zero, a
        # gradient routed through a window whose maximum occurs again after its first site
        w1, w2 = windows(r1), windows(r2_)
        ref["bites"] = {
            "out>0": int(((out == 0) & (go != 0)).sum()),
            "pool2>0": int(((p2 == 0) & (dp2 != 0)).sum()),
            "pool1>0": int(((p1 == 0) & (dp1 != 0)).sum()),
            "tie2": int((((w2 == p2[..., None]).sum(-1) > 1) & (p2 > 0) & (dp2 != 0)).sum()),
            "tie1": int((((w1 == p1[..., None]).sum(-1) > 1) & (p1 > 0) & (dp1 != 0)).sum())}
    for n, a in ref.items():
        if isinstance(a, np.ndarray):
            if a.dtype == np.float64:
                ref[n] = a = a + 0.0                # a sum of products 0 * -1 may come out as -0.0: the kernels' chains start at +0.0
            a.setflags(write=False)
    return ref


def sq_slices(grads):
    """float64 sums of squares of each SQ_GROUP-element slice of dk1 | db1 | dk2 | db2 | dk3 | db3 (the last one ragged)"""
    flat = np.concatenate([np.asarray(g, np.float64).reshape(-1) for g in grads])
    return np.array([np.square(flat[i:i + SQ_GROUP]).sum() for i in range(0, flat.size, SQ_GROUP)])


COMPARED = ["out", "pool1", "pool2", "d_images"] + NAMES        # every float tensor of an exact case must hold a non-zero


# ---------------------------------------------------------------------------------------------------------------- inputs
def _exact_inputs(seed, B, S, F):
    rng = np.random.RandomState(seed)
    taps = np.array([-1.0, 0.0, 0.0, 1.0], f32)
    P, c = {}, 1
    for i in (1, 2, 3):
        P["cnn/conv%d/kernel" % i] = taps[rng.randint(0, 4, (5, 5, c, F))]
        P["cnn/conv%d/bias" % i] = rng.randint(-1, 2, F).astype(f32)
        c = F
    images = rng.randint(0, 4, (B, S * S)).astype(f32)
    d_out = taps[rng.randint(0, 4, (B, (S // 4) ** 2 * F))]
    return P, images, d_out


def exact_ok(ref):
    """the conditions an exact case must meet: a non-zero in every compared tensor, every chain below 2^24 and, from S = 13
    up (the smallest planes have too few sites), at least one site of each of the five kinds `bites` counts"""
    S1 = ref["pool1"].shape[1]
    return (all(np.any(ref[n] != 0) for n in COMPARED) and max(ref["bounds"].values()) < EXACT_LIMIT
            and (S1 < 6 or min(ref["bites"].values()) > 0))


@functools.lru_cache(maxsize=None)
def exact_seed(B, S, F):
    """the first seed from 0 upward whose draw meets exact_ok (at S = 4..7 most draws leave a gradient all zero)"""
    for seed in range(5000):
        P, images, d_out = _exact_inputs(seed, B, S, F)
        if exact_ok(reference(P, images, d_out)):
            return seed
    raise AssertionError("no exact-integer draw for %r" % ((B, S, F),))


def _freeze(P, *arrays):
    for a in list(P.values()) + list(arrays):
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def exact_case(B, S, F):
    """(variables, images [B, S * S], d_out, float64 reference): computed once, read-only"""
    P, images, d_out = _exact_inputs(exact_seed(B, S, F), B, S, F)
    _freeze(P, images, d_out)
    return P, images, d_out, reference(P, images, d_out)


def variables(seed, F):
    """tests/test_gpu_cnn.py's _variables: Glorot-uniform kernels, biases in [-0.1, 0.1)"""
    rng = np.random.RandomState(seed)
    c = 1
    P = {}
    for i in (1, 2, 3):
        lim = np.sqrt(6.0 / (25 * c + 25 * F))
        P["cnn/conv%d/kernel" % i] = rng.uniform(-lim, lim, (5, 5, c, F)).astype(f32)
        P["cnn/conv%d/bias" % i] = rng.uniform(-0.1, 0.1, F).astype(f32)
        c = F
    return P


def _real_inputs(seed, B, S, F):
    """tests/test_gpu_cnn.py's _case: rows are drawn one after the other, so the first b images of a seed are its case at B = b"""
    images = np.random.RandomState(1000 + seed).uniform(0, 1, (B, S * S)).astype(f32)
    d_out = np.random.RandomState(2000 + seed).randn(B, (S // 4) ** 2 * F).astype(f32)   # what the device is given, exactly
    return variables(seed, F), images, d_out


def margins_ok(ref):
    """the precondition of a real-valued backward comparison: both margins, a live forward (below) and a non-zero in every
    compared tensor (at F = 1 a draw can leave the whole block dead: all gradients zero, nothing compared)"""
    return (ref["relu_margin"] >= MARGIN and ref["pool_margin"] >= MARGIN and live_ok(ref)
            and all(np.any(ref[n] != 0) for n in COMPARED if n in ref))


@functools.lru_cache(maxsize=None)
def real_seed(B, S, F):
    for seed in range(1, 200):
        if margins_ok(reference(*_real_inputs(seed, B, S, F))):
            return seed
    raise AssertionError("no seed meets the precondition at %r" % ((B, S, F),))


@functools.lru_cache(maxsize=None)
def real_case(B, S, F, seed=None):
    """(variables, images, d_out, reference); seed None: the first that meets the precondition at this (B, S, F)"""
    P, images, d_out = _real_inputs(real_seed(B, S, F) if seed is None else seed, B, S, F)
    _freeze(P, images, d_out)
    ref = reference(P, images, d_out)
    assert margins_ok(ref), (ref["relu_margin"], ref["pool_margin"])
    return P, images, d_out, ref


LIVE = 0.25


def live_ok(ref):
    """at least a quarter of out, pool1 and pool2 is positive.  The bound of a forward comparison is relative to the tensor's
    largest value; with F = 1 or 2 a draw can leave conv3 all but dead (0.2 % positive, the largest value 0.03 beside terms of
    0.3), and then that yardstick measures the cancellation of the draw, not the kernel"""
    return min(float((ref[n] > 0).mean()) for n in ("out", "pool1", "pool2")) >= LIVE


@functools.lru_cache(maxsize=None)
def real_forward_seed(B, S, F):
    for seed in range(1, 200):
        P, images, _ = _real_inputs(seed, B, S, F)
        if live_ok(reference(P, images)):
            return seed
    raise AssertionError("no live forward at %r" % ((B, S, F),))


@functools.lru_cache(maxsize=None)
def real_forward_case(B, S, F):
    """(variables, images, float64 forward reference) at the first seed with a live output: no margin precondition, the
    forward alone is compared"""
    P, images, _ = _real_inputs(real_forward_seed(B, S, F), B, S, F)
    _freeze(P, images)
    return P, images, reference(P, images)


# ----------------------------------------------------------------------------------------------------------- case tables
ALL_F = list(range(1, 9))
# every template instantiation: S = 13 -> 6 -> 3 (a dropped row, then an odd plane).  Real-valued only where
# tests/test_gpu_cnn.py has no real-valued case yet (it runs F = 3, 5, 8)
INSTANTIATION_EXACT = [(2, 13, F) for F in ALL_F]
INSTANTIATION_REAL = [(3, 13, F) for F in (1, 2, 4, 6, 7)]
# the declared limits (the last canvas of every filter count) and, at F = 8, the two sides of the "compact + codes" choice.
# It depends on S1 and its parity (the haloed pitch is even): compact + codes wins at S1 = 34, 36, 38 (S = 68, 69, 72, 73,
# 76, 77; by 8 floats only at S1 = 34), the haloed pool1 at every other S1 <= 38.  (69, 8) and (68, 8) take it, their
# nearest neighbours on either side, (70, 8) and (67, 8), do not.
LIMITS = [(2, S, F) for F, S in sorted(LAST_CANVAS.items(), reverse=True)]
COMPACT_EDGE = [(2, 69, 8), (2, 68, 8), (2, 70, 8), (2, 67, 8)]
# smallest planes: S2 = 1, S1 = 2, 2, 3, 3 -- every pixel of every plane sees padding
SMALLEST = [(B, S, F) for S in (4, 5, 6, 7) for F in (1, 8) for B in (1, 2)]
# thread-count edges: S1^2 = 256 windows is one pass of the forward's 256 threads, 289 one pass and 33; S^2 = 484 / 529
# straddle the backward's 512 threads in the d_images loop
THREAD_EDGES = [(2, 32, 4), (2, 34, 4), (2, 22, 4), (2, 23, 4)]
EXACT_CASES = INSTANTIATION_EXACT + LIMITS + COMPACT_EDGE + SMALLEST + THREAD_EDGES
REAL_FORWARD_CASES = LIMITS + COMPACT_EDGE
# batch reduction: B - 1 = 0, 1, 7, 8, 9, 16 additions against cnn_reduce_sq_kernel's unroll by 8; one seed, the first whose
# 17 images meet the precondition, so every B is a prefix of the same images and the single-image launches are shared
BATCH_S, BATCH_F, BATCH_MAX = 9, 3, 17
BATCH_SIZES = [1, 2, 8, 9, 10, 17]
# d_images = NULL and the forward without its saved tensors: one limit case, one smallest case
OPTIONAL_CASES = [(2, 77, 8), (1, 4, 1)]


def batch_case(B):
    return real_case(B, BATCH_S, BATCH_F, seed=real_seed(BATCH_MAX, BATCH_S, BATCH_F))
