"""Case tables, input builders and references for the pointwise kernels of csrc/air_pointwise.hip (tests/test_gpu_pointwise_edges.py
runs them on the device, tests/test_pointwise_edge_cases.py pins the tables and the references on the CPU).

Every kernel of the family runs 256 threads per workgroup and one thread per element, so the shape edges are sizes around
multiples of 256, R or Z equal to 1 and odd R or Z (the b = idx / R split).  The two element-wise launchers cap their grid at
2048 workgroups and stride over the rest; their long cases lie just past one pass of that grid.

Per kernel there are two host statements of the same operation on the SAME fp32 inputs:
  *_ref  float64 on the inputs widened: what the device result is compared with;
  *_f32  numpy fp32 in the kernel's own operation order: what a correct fp32 kernel computes up to its libm.
The bounds are the suite's own (the names below say where each comes from).  The inputs are sized for them: on the CPU,
*_f32 lies within QUARTER of every bound of *_ref for every case (test_pointwise_edge_cases.py), which leaves three quarters
for the device's tanhf, expf, logf and sqrtf.  That is a condition on the inputs; no element of a result is filtered.

Inputs of a backward case come from the float64 forward rounded to fp32, never from a forward launch."""
import numpy as np

from air import _hip as H
from step_limit_cases import dyn_vector

THREADS = 256                                     # per workgroup, in every kernel of the file
GRID_CAP = 2048                                   # workgroups of reparam_bwd_plain_kernel and ew_launch
QUARTER = 0.25

# ---- the bounds (|got - ref| <= atol + rtol |ref|) ----------------------------------------------------------------------
LSTM_FWD_TOL = (2e-6, 2e-6)                       # (rtol, atol) test_unfused_lstm_and_reparam_kernels_match_oracle
LSTM_BWD_TOL = (2e-5, 2e-6)                       # the same test, backward of the cell
REPARAM_FWD_TOL = (2e-6, 2e-6)                    # the same test
REPARAM_BWD_TOL = (0.0, 2e-5)                     # the fused-epilogue bound of tests/test_gpu_gemm_edges.py, absolute
BCE_LOSS_TOL = (2e-5, 0.0)                        # test_bce_fwd_bwd_matches_oracle_formula
BCE_GRAD_TOL = (2e-4, 1e-7)                       # the same test
# the batch mean of finalize_kernel: additions on the longest path of a sum of POSITIVE terms, each of relative error 2^-24
# of a partial sum that is at most the total:
#   1 (L + rec_loss)  +  ceil(B / 256) (the thread's loop)  +  6 (butterfly levels)  +  3 (wave sums)  +  1 (the division)
MEAN_FIXED_OPS = 1 + 6 + 3 + 1


def mean_bound(B, mean):
    return (-(-B // THREADS) + MEAN_FIXED_OPS) * 2.0 ** -24 * mean


def ratio(got, ref, tol):
    """largest |got - ref| / (atol + rtol |ref|); inf where a value is not finite"""
    rtol, atol = tol
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not np.isfinite(got).all():
        return np.inf
    return float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())


# ---- case tables --------------------------------------------------------------------------------------------------------
LSTM_FWD_SHAPES = [(1, 1), (3, 5), (1, 256), (2, 256), (257, 1), (5, 103), (37, 24), (64, 256)]
FIRST_STEP_SHAPES = [(3, 5), (37, 24), (64, 256)]
FIRST_STEP_CASES = [dict(B=B, R=R, nslabs=n, bias=bias, h16=h16)
                    for (B, R) in FIRST_STEP_SHAPES for n in range(1, 9) for bias in (True, False) for h16 in (True, False)]
LSTM_BWD_SHAPES = [(1, 1), (3, 5), (257, 1), (37, 24), (64, 256)]
DGSUM_MODES = ("absent", "stored", "accumulated")
LSTM_BWD_CASES = [dict(B=B, R=R, dc_in=dc, dgsum=mode) for (B, R) in LSTM_BWD_SHAPES for dc in (True, False) for mode in DGSUM_MODES]
REPARAM_SHAPES = [(1, 1), (5, 2), (256, 1), (3, 257), (37, 50), (64, 50)]
PLAIN_SHAPES = [(1, 1), (5, 2), (37, 50), (2049, 256)]    # the last: 524 544 elements, 256 past one pass of 2048 x 256 threads
PLAIN_CASES = [dict(M=M, Z=Z, d_mean_in=dm, d_lv_in=dl) for (M, Z) in PLAIN_SHAPES for dm in (True, False) for dl in (True, False)]
SIGMOID_N = [1, 3, 4, 5, 1027, 4 * 524288 + 7]             # the last: a second pass of the 16-byte body plus a scalar tail
SIGMOID_OFF = [(0, 0, 0), (4, 0, 0), (0, 4, 0), (0, 0, 4)]  # bytes (d_rec, rec, d_pre) lie behind a 16-byte boundary
SIGMOID_CASES = [dict(n=n, off=off) for n in SIGMOID_N for off in SIGMOID_OFF]
BCE_SHAPES = [(5, 2500), (2, 1), (3, 257), (1, 256), (4, 255)]
BCE_CASES = [dict(B=B, D=D, d_recon=dr) for (B, D) in BCE_SHAPES for dr in (True, False)]
BCE_TIES = np.array([0.0, 1.0, -0.0, 0.5, 1.0000001, -1e-8, 0.25], np.float32)    # test_bce_fwd_bwd_matches_oracle_formula's
FINALIZE_B = [1, 2, 255, 256, 257, 1000]


def finalize_cases():
    """B x (all targets equal their digit, none, k of them for a k that does not divide B: there is none for B = 1, 2)"""
    out = []
    for B in FINALIZE_B:
        ks = [B, 0]
        k = 2 * B // 3
        while k > 1 and B % k == 0:
            k -= 1
        if k > 1:
            ks.append(k)
        out += [dict(B=B, k=k) for k in ks]
    return out


def describe(c):
    return " ".join("%s=%s" % kv for kv in c.items())


def _seed(tag, *nums):
    """a RandomState per (kernel, shape): tag is the kernel's number in this file"""
    return np.random.RandomState([int(tag)] + [int(n) for n in nums])


def bf16_bits(x):
    """round-to-nearest-even bf16 bit patterns (int16) of finite fp32 values"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16).view(np.int16)


def nan_record(shape, fields):
    """a record array that is NaN except `fields` = {column: values}"""
    a = np.full(shape, np.nan, np.float32)
    for col, v in fields.items():
        a[..., col] = v
    return a


def dyn_only(B, *slots):
    """the AIR_DYN_* vector of step_limit_cases.dyn_vector(B) with every slot but `slots` NaN"""
    full = dyn_vector(B)
    return nan_record((H.DYN_COUNT,), {s: full[s] for s in slots})


# ---- the LSTM cell ------------------------------------------------------------------------------------------------------
def lstm_fwd_inputs(B, R, tag=1):
    rng = _seed(tag, B, R)
    return dict(pre=rng.uniform(-6, 6, (B, 4 * R)).astype(np.float32), c_prev=rng.uniform(-1, 1, (B, R)).astype(np.float32))


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_fwd_ref(pre, c_prev):
    """(acts [B, 4R], c, h) of BasicLSTMCell in float64: gates i, j, f, o, forget bias 1.0"""
    i, j, f, o = np.split(pre.astype(np.float64), 4, axis=1)
    si, tj, sf, so = _sigmoid(i), np.tanh(j), _sigmoid(f + 1.0), _sigmoid(o)
    c = c_prev.astype(np.float64) * sf + si * tj
    return np.concatenate([si, tj, sf, so], 1), c, np.tanh(c) * so


def lstm_fwd_f32(pre, c_prev):
    """air_lstm_cell_fwd in numpy fp32, in its order: 1 / (1 + exp(-x)); c * sf + si * tj; tanh(c') * so"""
    one = np.float32(1.0)
    i, j, f, o = np.split(pre, 4, axis=1)
    sig = lambda x: one / (one + np.exp(-x))  # noqa: E731
    si, tj, sf, so = sig(i), np.tanh(j), sig(f + one), sig(o)
    c = c_prev * sf + si * tj
    return np.concatenate([si, tj, sf, so], 1), c, np.tanh(c) * so


def first_step_inputs(c):
    """slabs [nslabs, B, 4R] uniform in +-1.5, slab k scaled by 10^(-3 .. 0) (ascending, so the last slab is the large one and
    every earlier partial sum is rounded at another magnitude than in any other order); bias [4R] uniform in +-0.5"""
    B, R, n = c["B"], c["R"], c["nslabs"]
    rng = _seed(2, B, R, n)
    scale = 10.0 ** (-3.0 + 3.0 * np.arange(1, n + 1) / n)
    slabs = (rng.uniform(-1.5, 1.5, (n, B, 4 * R)) * scale[:, None, None]).astype(np.float32)
    return dict(slabs=slabs, bias=rng.uniform(-0.5, 0.5, 4 * R).astype(np.float32))


def first_step_pre(slabs, bias, order=None):
    """((0 + s0) + s1) ... + bias in fp32: the order lstm_first_step_kernel and the fused epilogue promise"""
    s = np.zeros(slabs.shape[1:], np.float32)
    for k in (range(slabs.shape[0]) if order is None else order):
        s = s + slabs[k]
    return s if bias is None else s + bias[None, :]


def lstm_bwd_inputs(B, R):
    """acts and c are the float64 forward rounded to fp32; dh and dc_in normal, clipped at +-3; dgsum's initial values normal"""
    f = lstm_fwd_inputs(B, R, tag=3)
    rng = _seed(4, B, R)
    acts, c, _ = lstm_fwd_ref(f["pre"], f["c_prev"])
    return dict(acts=acts.astype(np.float32), c=c.astype(np.float32), c_prev=f["c_prev"],
                dh=np.clip(rng.randn(B, R), -3, 3).astype(np.float32), dc_in=np.clip(rng.randn(B, R), -3, 3).astype(np.float32),
                dgsum0=rng.randn(B, 4 * R).astype(np.float32))


def _lstm_bwd(x, dc_in, t):
    one = t(1.0)
    si, tj, sf, so = np.split(x["acts"].astype(t), 4, axis=1)
    tc = np.tanh(x["c"].astype(t))
    dh = x["dh"].astype(t)
    dc = (x["dc_in"].astype(t) if dc_in else t(0.0)) + dh * so * (one - tc * tc)
    dgi = dc * tj * si * (one - si)
    dgj = dc * si * (one - tj * tj)
    dgf = dc * x["c_prev"].astype(t) * sf * (one - sf)
    dgo = dh * tc * so * (one - so)
    return np.concatenate([dgi, dgj, dgf, dgo], 1), dc * sf


def lstm_bwd_ref(x, dc_in):
    """(dgates [B, 4R], dc_prev) in float64"""
    return _lstm_bwd(x, dc_in, np.float64)


def lstm_bwd_f32(x, dc_in):
    """lstm_gates_bwd_kernel's expressions, left to right, in numpy fp32"""
    return _lstm_bwd(x, dc_in, np.float32)


# ---- re-parameterisation ------------------------------------------------------------------------------------------------
def reparam_inputs(B, Z):
    """ml = mean (+-2) | log-variance (-6 .. 2); eps and d_zs normal, clipped at +-3; mask rows 0 and 1, both present when
    B > 1; att and dyn are NaN in every field the kernel has no business with"""
    rng = _seed(5, B, Z)
    ml = np.concatenate([rng.uniform(-2, 2, (B, Z)), rng.uniform(-6, 2, (B, Z))], 1).astype(np.float32)
    mask = (rng.uniform(size=B) < 0.5).astype(np.float32)
    if B > 1:
        mask[0], mask[-1] = 1.0, 0.0
    else:
        mask[0] = 1.0
    return dict(ml=ml, eps=np.clip(rng.randn(B, Z), -3, 3).astype(np.float32), d_zs=np.clip(rng.randn(B, Z), -3, 3).astype(np.float32),
                mask=mask, att=nan_record((B, H.ATT_STRIDE), {H.ATT_MASK: mask}),
                dyn=dyn_only(B, H.DYN_GRAD_SCALE, H.DYN_VAE_PV, H.DYN_VAE_PM))


def _reparam_fwd(x, t):
    Z = x["eps"].shape[1]
    ml = x["ml"].astype(t)
    return ml[:, :Z] + x["eps"].astype(t) * np.sqrt(np.exp(ml[:, Z:]))


def reparam_fwd_ref(x):
    return _reparam_fwd(x, np.float64)


def reparam_fwd_f32(x):
    return _reparam_fwd(x, np.float32)


def _reparam_bwd(x, t):
    """mean leg d + klg (mean - pm) / pv; log-variance leg d eps sd / 2 + klg (var / pv - 1) / 2; klg = mask grad_scale"""
    Z = x["eps"].shape[1]
    ml, d, eps = x["ml"].astype(t), x["d_zs"].astype(t), x["eps"].astype(t)
    dyn = x["dyn"].astype(t)
    klg = (x["mask"].astype(t) * dyn[H.DYN_GRAD_SCALE])[:, None]
    pv, pm = dyn[H.DYN_VAE_PV], dyn[H.DYN_VAE_PM]
    var = np.exp(ml[:, Z:])
    sd = np.sqrt(var)
    half, one = t(0.5), t(1.0)
    return np.concatenate([d + klg * (ml[:, :Z] - pm) / pv, d * eps * half * sd + klg * half * (var / pv - one)], 1)


def reparam_bwd_ref(x):
    return _reparam_bwd(x, np.float64)


def reparam_bwd_f32(x):
    return _reparam_bwd(x, np.float32)


def plain_inputs(M, Z):
    rng = _seed(6, M, Z)
    x = reparam_inputs(M, Z)
    return dict(ml=x["ml"], eps=x["eps"], d_zs=x["d_zs"], d_mean_in=np.clip(rng.randn(M, Z), -3, 3).astype(np.float32),
                d_lv_in=np.clip(rng.randn(M, Z), -3, 3).astype(np.float32))


def plain_mean_bits(x, d_mean_in):
    """the mean half: one fp32 addition, or a copy"""
    return x["d_zs"] + x["d_mean_in"] if d_mean_in else x["d_zs"].copy()


def _plain_lv(x, d_lv_in, t):
    Z = x["eps"].shape[1]
    gl = ((x["d_zs"].astype(t) * x["eps"].astype(t)) * t(0.5)) * np.sqrt(np.exp(x["ml"].astype(t)[:, Z:]))
    return gl + x["d_lv_in"].astype(t) if d_lv_in else gl


def plain_lv_ref(x, d_lv_in):
    return _plain_lv(x, d_lv_in, np.float64)


def plain_lv_f32(x, d_lv_in):
    return _plain_lv(x, d_lv_in, np.float32)


# ---- SigmoidGrad --------------------------------------------------------------------------------------------------------
def sigmoid_inputs(n):
    rng = _seed(7, n)
    return dict(g=rng.randn(n).astype(np.float32), r=rng.uniform(0, 1, n).astype(np.float32))


def sigmoid_bwd_bits(x):
    """(g r) (1 - r): no libm call and nothing an FMA could contract, so the device result has these bits"""
    return (x["g"] * x["r"]) * (np.float32(1.0) - x["r"])


# ---- Bernoulli cross-entropy --------------------------------------------------------------------------------------------
def bce_inputs(B, D):
    """test_bce_fwd_bwd_matches_oracle_formula's inputs at any shape: sparse images, a running reconstruction in (-0.2, 1.3)
    with the test's ties and just-outside values in front (as many as the array holds)"""
    rng = _seed(8, B, D)
    x = (rng.rand(B, D) * (rng.rand(B, D) > 0.8)).astype(np.float32)
    R = rng.uniform(-0.2, 1.3, size=(B, D)).astype(np.float32)
    k = min(BCE_TIES.size, B * D)
    R.reshape(-1)[:k] = BCE_TIES[:k]
    return dict(x=x, R=R, dyn=dyn_only(B, H.DYN_GRAD_SCALE))


def bce_recon_bits(x):
    return np.clip(x["R"], np.float32(0.0), np.float32(1.0))


def bce_ref(x):
    """(rec_loss [B], d_recon [B, D]) in float64, as test_bce_fwd_bwd_matches_oracle_formula: p1 and p0 are the fp32 values"""
    img, R = x["x"].astype(np.float64), x["R"]
    r = np.clip(R, np.float32(0.0), np.float32(1.0))
    p1, p0 = (r + np.float32(1e-9)).astype(np.float64), ((np.float32(1.0) - r) + np.float32(1e-9)).astype(np.float64)
    loss = -np.sum(img * np.log(p1) + (1 - img) * np.log(p0), axis=1)
    g = -(img / p1 - (1 - img) / p0) * float(x["dyn"][H.DYN_GRAD_SCALE])
    g[(R > 1.0) | (R < 0.0)] = 0.0                                      # clipped away: no gradient
    return loss, g


def _block_sum_256(v):
    """air_block_sum_256 of 256 per-thread values in fp32: a 6-level xor butterfly per wave, then ((w0 + w1) + w2) + w3"""
    w = np.asarray(v, np.float32).reshape(4, 64).copy()
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ off]
    return ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]


def _thread_sums(terms):
    """per thread t the fp32 sum of terms[t], terms[t + 256], ... in that order, from 0.0"""
    acc = np.zeros(THREADS, np.float32)
    for k0 in range(0, terms.size, THREADS):
        part = terms[k0:k0 + THREADS]
        acc[:part.size] = acc[:part.size] + part
    return acc


def bce_f32(x):
    """bce_kernel in numpy fp32: (rec_loss, d_recon)"""
    one, eps = np.float32(1.0), np.float32(1e-9)
    img, R = x["x"], x["R"]
    gsc = x["dyn"][H.DYN_GRAD_SCALE]
    r = np.maximum(np.minimum(R, one), np.float32(0.0))
    p1, p0 = r + eps, (one - r) + eps
    term = img * np.log(p1) + (one - img) * np.log(p0)
    loss = np.array([-_block_sum_256(_thread_sums(term[b])) for b in range(R.shape[0])], np.float32)
    g = np.where((R <= one) & (np.minimum(R, one) >= 0), -gsc * (img / p1 - (one - img) / p0), np.float32(0.0))
    return loss, g.astype(np.float32)


# ---- batch means --------------------------------------------------------------------------------------------------------
def finalize_inputs(c):
    """run_loss in (50, 900), rec_loss in (100, 2000); k of the B targets (at random places) equal their digit"""
    B, k = c["B"], c["k"]
    rng = _seed(9, B, k)
    digits = rng.randint(0, 4, B).astype(np.int32)
    targets = digits + 1
    targets[rng.permutation(B)[:k]] -= 1
    return dict(run_loss=rng.uniform(50, 900, B).astype(np.float32), rec_loss=rng.uniform(100, 2000, B).astype(np.float32),
                targets=targets.astype(np.int32), digits=digits)


def finalize_ref(x):
    """the float64 mean of run_loss + rec_loss"""
    return float((x["run_loss"].astype(np.float64) + x["rec_loss"].astype(np.float64)).mean())


def finalize_f32(x):
    """finalize_kernel in numpy fp32: (loss_per_item, mean loss, accuracy)"""
    item = x["run_loss"] + x["rec_loss"]
    B = np.float32(item.size)
    hit = (x["targets"] == x["digits"]).astype(np.float32)
    return item, _block_sum_256(_thread_sums(item)) / B, _block_sum_256(_thread_sums(hit)) / B
