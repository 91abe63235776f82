"""Inputs and fp64 references for the step-limit tests (tests/test_gpu_step_limits.py, tests/test_step_limit_cases.py).

The attend and compose kernels are driven through the C ABI at N = 16 steps with inputs built HERE, not by a model: the
test decides, per (step, image), the seven head outputs -- so which image is still alive at which step is a property of the
input, known before any kernel runs -- and every comparison is kept away from the discontinuities of the step logic
(S < threshold, round(z_pres), the clip of a tap at the border of its source).  The margins are conditions on the INPUTS,
computed from the fp64 reference alone and asserted by tests/test_step_limit_cases.py on the CPU; no result is filtered.

The reference restates the step loop of the oracle (oracle/air_oracle.py air_forward, the body between the LSTM and the
VAE: air_model.py:288-333, 368-427, 441-477 of the reference) from the oracle's own pieces in float64: ao.transformer,
ao.concrete_binary_pre_sigmoid_sample, ao.concrete_binary_kl_mc_sample, ao._gauss_kl, ao.sigmoid."""
import functools

import numpy as np

from air import _hip as H
from oracle import air_oracle as ao
from oracle.synth import blob_canvases

N_STEPS = 16
# the step at which image b stops (S >= threshold AFTER that step; None: alive through all 16 steps)
STOPS_B4 = (None, 0, 7, 15)
STOPS_B3 = (None, 7, 15)

THRESHOLD, TEMPERATURE, PRIOR_LOG_ODDS = 0.99, 0.8, -2.0
S_MARGIN = 1e-3          # |S - threshold| before and after every step
ROUND_MARGIN = 1e-3      # |sigmoid(z_pre) - 0.5| in eval mode
TAP_MARGIN = 1e-3        # distance (in source pixels) of every tap coordinate from the two clip edges 0 and n_in - 1
SCALE_RANGE = (0.2, 1.2)
BAND = 1e-4              # d_recon is compared where the fp64 running reconstruction is this far from 0 and from 1
ILL = 1e-3               # the images of a compose case carry no free ink within this of the two poles (see write_case)

ATTEND_SHAPES = [(50, 28), (51, 28), (40, 9), (128, 32), (64, 64), (7, 2)]
HEAD_SHAPES = [(1, 1, 1), (5, 17, 33), (200, 200, 100), (256, 256, 256)]
# not the full product: (50, 28) and (51, 28) -- the two sides of the C * C <= 2560 staging threshold -- with every head
# shape, every other canvas with one head shape each (every value appears); each of them with train = 0 and 1
ATTEND_CASES = ([(C, w, h) for (C, w) in ATTEND_SHAPES[:2] for h in HEAD_SHAPES] +
                [(40, 9, (5, 17, 33)), (128, 32, (200, 200, 100)), (64, 64, (1, 1, 1)), (7, 2, (256, 256, 256))])
WRITE_CASES = ([(C, w, 50) for (C, w) in [(50, 28), (51, 28), (64, 32), (65, 32), (33, 7)]] +
               [(50, 28, 1), (51, 28, 65), (33, 7, 130), (65, 32, 130)])


def dyn_vector(B):
    """the AIR_DYN_* array of the kernels (fp32), training.py's priors"""
    dyn = np.zeros(H.DYN_COUNT, np.float32)
    dyn[H.DYN_PRIOR_LOG_ODDS], dyn[H.DYN_TEMPERATURE], dyn[H.DYN_STOP_THRESHOLD] = PRIOR_LOG_ODDS, TEMPERATURE, THRESHOLD
    dyn[H.DYN_SCALE_PM], dyn[H.DYN_SCALE_PV] = -1.0, 0.05
    dyn[H.DYN_SHIFT_PM], dyn[H.DYN_SHIFT_PV] = 0.25, 1.5
    dyn[H.DYN_VAE_PM], dyn[H.DYN_VAE_PV] = -0.125, 0.75
    dyn[H.DYN_LIK_STD], dyn[H.DYN_GRAD_SCALE] = 0.3, 1.0 / B
    for plv, pv in ((H.DYN_SCALE_PLV, H.DYN_SCALE_PV), (H.DYN_SHIFT_PLV, H.DYN_SHIFT_PV), (H.DYN_VAE_PLV, H.DYN_VAE_PV)):
        dyn[plv] = np.log(dyn[pv])                          # air_model.py:72-74: tf.log of the fp32 constant
    return dyn


def head_layout(Hs, Hh, Hz):
    """(offset, width) of the hidden segment each of the 7 output units reads (include/air_hip.h, air_attend_fwd_t)"""
    wid = (Hs, Hs, Hh, Hh, Hz)
    off = np.concatenate([[0], np.cumsum(wid)[:-1]])
    head_of = (0, 1, 2, 2, 3, 3, 4)
    return [(int(off[h]), int(wid[h])) for h in head_of]


def _logit(p):
    return np.log(p) - np.log1p(-p)


def _plan(rng, N, B, stops, train):
    """What every (step, image) should come out as: glimpse (s, x, y), the log-variances and the z_pres log-odds"""
    s = rng.uniform(0.22, 0.95, (N, B))
    x = rng.uniform(-0.8, 0.8, (N, B))
    y = rng.uniform(-0.8, 0.8, (N, B))
    # the first four steps tile the canvas (four glimpses of scale ~0.85 around (+-0.25, +-0.25)): with them the running
    # reconstruction of a compose case is non-zero nearly everywhere, and they hang over the canvas edge (s + |x| > 1)
    for t, (qx, qy) in enumerate(((-1, -1), (1, -1), (-1, 1), (1, 1))):
        s[t] = rng.uniform(0.82, 0.92, B)
        x[t] = qx * rng.uniform(0.22, 0.28, B)
        y[t] = qy * rng.uniform(0.22, 0.28, B)
    lv = rng.uniform(-4.0, -1.0, (N, B, 3))                  # scale, shift x, shift y log-variances
    # z_pres log-odds: far on the "present" side while alive (the always-alive image adds ~1e-6 per step, the one that stops
    # at step 15 ~1e-2 per step: a sum that is not trivial in fp32 and stays below 0.55), far on the other side at the
    # stopping step, anything away from 0 afterwards
    lo = np.zeros((N, B))
    for b, stop in enumerate(stops):
        alive = 12.0 if stop is None else (4.0 if stop >= 12 else 9.0)
        for t in range(N):
            if stop is None or t < stop:
                lo[t, b] = alive + rng.uniform(-0.5, 0.5)
            elif t == stop:
                lo[t, b] = -8.0 + rng.uniform(-0.5, 0.5)
            else:
                lo[t, b] = rng.choice([-1.0, 1.0]) * rng.uniform(1.5, 3.0)
    return s, x, y, lv, lo


def _attend_case_once(C, w, heads, train, seed, B, stops, wout_ld, attempt):
    """fp32 inputs of air_attend_fwd at N = 16: hid [N,B,HT], wout [7,wout_ld], bout [7], canvas [B,C*C], noise, dyn.

    The hidden vector of (t, b) is a random mixed-sign vector plus the smallest correction (in the span of the weight rows
    of its segment) that makes the output units of that segment hit their planned values exactly -- in real arithmetic;
    after the rounding to fp32 the plan is met to ~1e-6, and the reference recomputes everything from the rounded inputs.
    A one-wide segment shared by two units (shift heads at Hh = 1) fixes the first unit only."""
    Hs, Hh, Hz = heads
    N = N_STEPS
    stops = stops or (STOPS_B4 if B == 4 else STOPS_B3)
    assert len(stops) == B
    rng = np.random.RandomState(1000 * C + 10 * w + Hs + 7 * train + 100003 * seed + 7919 * attempt)
    layout = head_layout(Hs, Hh, Hz)
    HT = 2 * Hs + 2 * Hh + Hz
    ld = wout_ld or max(heads)
    s, x, y, lv, lo = _plan(rng, N, B, stops, train)
    eps_scale = np.clip(rng.standard_normal((N, B, 1)), -2.5, 2.5).astype(np.float32)
    eps_shift = np.clip(rng.standard_normal((N, B, 2)), -2.5, 2.5).astype(np.float32)
    u = rng.uniform(0.3, 0.7, (N, B)).astype(np.float32)
    sd = np.sqrt(np.exp(lv))
    target = np.zeros((N, B, 7))
    target[..., 0] = _logit(s) - eps_scale[..., 0] * sd[..., 0]
    target[..., 1] = lv[..., 0]
    target[..., 2] = np.arctanh(x) - eps_shift[..., 0] * sd[..., 1]
    target[..., 3] = np.arctanh(y) - eps_shift[..., 1] * sd[..., 2]
    target[..., 4], target[..., 5] = lv[..., 1], lv[..., 2]
    target[..., 6] = lo
    wout = np.full((7, ld), np.nan)                         # the pad of a row is never read into a product
    for o, (_, wid) in enumerate(layout):
        wout[o, :wid] = rng.uniform(0.25, 1.0, wid) * rng.choice([-1.0, 1.0], wid) / np.sqrt(wid)
    if Hh == 1:                                             # y rides on x (one hidden unit, two outputs): keep it in range
        wout[3, 0], wout[5, 0] = -0.7 * wout[2, 0], 0.9 * wout[4, 0]
    bout = rng.uniform(-0.3, 0.3, 7)
    if Hh == 1:
        bout[5] = bout[4] * 0.9 - 0.2
    # Weights and the free part of the hidden vector shrink with 1 / sqrt(width), as Glorot weights do: the products of a
    # unit then sum to about its planned value instead of cancelling from a sum of |terms| ~ width / 5.  It matters because
    # the glimpse amplifies: d window = |grad canvas| * (C - 1.001) / 2 * d(s, x, y) -- 64 x at C = 128 -- so the fp32
    # summation error of an ill-conditioned 256-term product (1e-6 in x, measured) would be judged, not the kernel
    hid = rng.uniform(-1.0, 1.0, (N, B, HT))
    for off, wid in set(layout):
        hid[..., off:off + wid] /= np.sqrt(wid)
    for units in ((0,), (1,), (2, 3), (4, 5), (6,)):
        off, wid = layout[units[0]]
        units = units[:min(len(units), wid)]
        W = wout[list(units), :wid]                          # [k, wid]
        r = hid[..., off:off + wid]
        miss = target[..., list(units)] - bout[list(units)] - r @ W.T
        hid[..., off:off + wid] = r + miss @ np.linalg.solve(W @ W.T, W)
    rngc = np.random.RandomState(seed + 17)
    canvas, _ = blob_canvases(B, C, 2, seed=seed + 3) if C >= 20 else (np.zeros((B, C * C), np.float32), None)
    canvas = np.clip(canvas + rngc.uniform(0.0, 0.3, canvas.shape), 0.0, 1.0).astype(np.float32)   # no flat regions
    return dict(C=C, w=w, heads=heads, train=train, N=N, B=B, HT=HT, wout_ld=ld, stops=stops,
                hid=hid.astype(np.float32), wout=wout.astype(np.float32), bout=bout.astype(np.float32), canvas=canvas,
                eps_scale=eps_scale, eps_shift=eps_shift, u=u, dyn=dyn_vector(B))


def _margins_met(case, m):
    return (m["S"] >= S_MARGIN and (case["train"] or m["round"] >= ROUND_MARGIN) and m["tap"] >= TAP_MARGIN and
            SCALE_RANGE[0] <= m["scale_min"] and m["scale_max"] <= SCALE_RANGE[1])


@functools.lru_cache(maxsize=None)
def attend_case_and_reference(C, w, heads, train, seed=0, B=4, stops=None, wout_ld=None):
    """(case, fp64 reference) -- built once per process and shared: treat both as read-only.  A draw whose reference misses a
    margin (a tap coordinate within 1e-3 of a clip edge happens once in a few dozen draws) is drawn again: the builder
    meets the conditions, no comparison is dropped."""
    for attempt in range(16):
        case = _attend_case_once(C, w, heads, train, seed, B, stops, wout_ld, attempt)
        ref = attend_reference(case)
        if _margins_met(case, attend_margins(case, ref)):
            return case, ref
    raise AssertionError("no draw meets the margins: change the builder")


def attend_case(C, w, heads, train, seed=0, B=4, stops=None, wout_ld=None):
    return attend_case_and_reference(C, w, heads, train, seed, B, stops, wout_ld)[0]


def restride_wout(case, wout_ld):
    """the same case with the rows of wout at another stride, the pad filled with NaN"""
    wout = np.full((7, wout_ld), np.nan, np.float32)
    k = min(wout_ld, case["wout_ld"])
    wout[:, :k] = case["wout"][:, :k]
    return dict(case, wout=wout, wout_ld=wout_ld)


def _dyn64(dyn):
    return {k: np.float64(dyn[getattr(H, "DYN_" + k)]) for k in
            ("PRIOR_LOG_ODDS", "TEMPERATURE", "STOP_THRESHOLD", "SCALE_PM", "SCALE_PV", "SHIFT_PM", "SHIFT_PV", "VAE_PM", "VAE_PV",
             "GRAD_SCALE", "SCALE_PLV", "SHIFT_PLV", "VAE_PLV")}


def attend_reference(case):
    """The step loop of ao.air_forward between the LSTM and the VAE in float64, on the case's fp32 inputs.
    Returns out7 [N,B,8], att [N,B,16], window [N,B,w*w] and the margins of the step logic:
    S_before / S_after [N,B], z_sigmoid [N,B] (before tf.round), tap_x / tap_y: the source coordinates of every tap."""
    f = np.float64
    N, B, C, w = case["N"], case["B"], case["C"], case["w"]
    d = _dyn64(case["dyn"])
    hid, wout, bout = case["hid"].astype(f), case["wout"].astype(f), case["bout"].astype(f)
    canvas = case["canvas"].astype(f).reshape(B, C, C)
    out7 = np.zeros((N, B, H.OUT_STRIDE), f)
    for o, (off, wid) in enumerate(head_layout(*case["heads"])):
        out7[..., o] = hid[..., off:off + wid] @ wout[o, :wid] + bout[o]
    att = np.zeros((N, B, H.ATT_STRIDE), f)
    window = np.zeros((N, B, w * w), f)
    S = np.zeros(B, f)
    S_before, S_after, zsig = np.zeros((N, B), f), np.zeros((N, B), f), np.zeros((N, B), f)
    tap_x, tap_y = [], []
    thr, T = d["STOP_THRESHOLD"], d["TEMPERATURE"]
    for t in range(N):
        o = out7[t]
        # scale :288-303, shift :305-320
        scale_mean, scale_lv = o[:, 0:1], o[:, 1:2]
        scale_var = np.exp(scale_lv)
        s = ao.sigmoid(scale_mean + case["eps_scale"][t].astype(f) * np.sqrt(scale_var))[:, 0]
        shift_mean, shift_lv = o[:, 2:4], o[:, 4:6]
        shift_var = np.exp(shift_lv)
        shift = np.tanh(shift_mean + case["eps_shift"][t].astype(f) * np.sqrt(shift_var))
        x, y = shift[:, 0], shift[:, 1]
        # st_forward :322-333
        zeros = np.zeros_like(s)
        theta = np.stack([np.stack([s, zeros, x], axis=1), np.stack([zeros, s, y], axis=1)], axis=1)
        win, aux = ao.transformer(canvas, theta, (w, w), return_aux=True)
        tap_x.append(aux["x"]), tap_y.append(aux["y"])
        # z_pres :368-396
        z_lo = o[:, 6]
        z_pre = ao.concrete_binary_pre_sigmoid_sample(z_lo, T, case["u"][t].astype(f))
        z = ao.sigmoid(z_pre)
        zsig[t] = z
        if not case["train"]:
            z = np.round(z)
        z_kl = ao.concrete_binary_kl_mc_sample(z_pre, d["PRIOR_LOG_ODDS"], T, z_lo, T)
        # stop logic :409-427
        S_before[t] = S
        mask_prev = S < thr
        S = S + (f(1.0) - z)
        S_after[t] = S
        mask = S < thr
        scale_kl = ao._gauss_kl(d["SCALE_PLV"], scale_lv, scale_var, d["SCALE_PV"], scale_mean, d["SCALE_PM"])
        shift_kl = ao._gauss_kl(d["SHIFT_PLV"], shift_lv, shift_var, d["SHIFT_PV"], shift_mean, d["SHIFT_PM"])
        a = att[t]
        a[:, H.ATT_S], a[:, H.ATT_X], a[:, H.ATT_Y] = s, x, y
        a[:, H.ATT_ZPRE], a[:, H.ATT_Z], a[:, H.ATT_ZPROB] = z_pre, z, ao.sigmoid(z_lo)
        a[:, H.ATT_KL_Z], a[:, H.ATT_KL_SCALE], a[:, H.ATT_KL_SHIFT] = z_kl, scale_kl, shift_kl
        a[:, H.ATT_MASK_PREV], a[:, H.ATT_MASK] = mask_prev, mask
        a[:, H.ATT_ST_BACK], a[:, H.ATT_ST_BACK + 1], a[:, H.ATT_ST_BACK + 2] = 1.0 / s, -x / s, -y / s
        window[t] = win.reshape(B, w * w)
    return dict(out7=out7, att=att, window=window, S_before=S_before, S_after=S_after, z_sigmoid=zsig,
                tap_x=np.stack(tap_x), tap_y=np.stack(tap_y))


def tap_margin(coords, n_in):
    """smallest distance of a tap coordinate from the two places where the clipped bilinear read jumps: 0 and n_in - 1"""
    c = np.asarray(coords, np.float64)
    return float(min(np.abs(c).min(), np.abs(c - (n_in - 1)).min()))


def attend_margins(case, ref):
    """the conditions of the inputs (all from the fp64 reference): see tests/test_step_limit_cases.py"""
    thr = float(case["dyn"][H.DYN_STOP_THRESHOLD])
    m = dict(S=float(min(np.abs(ref["S_before"] - thr).min(), np.abs(ref["S_after"] - thr).min())),
             round=float(np.abs(ref["z_sigmoid"] - 0.5).min()),
             tap=min(tap_margin(ref["tap_x"], case["C"]), tap_margin(ref["tap_y"], case["C"])),
             scale_min=float(ref["att"][..., H.ATT_S].min()), scale_max=float(ref["att"][..., H.ATT_S].max()))
    s, x, y = (ref["att"][..., k] for k in (H.ATT_S, H.ATT_X, H.ATT_Y))
    m["overhang"] = int(((s + np.abs(x) > 1.0) | (s + np.abs(y) > 1.0)).sum())
    return m


def expected_masks(stops, N=N_STEPS):
    """MASK_PREV / MASK [N,B] of a stop plan: an image that stops at step k has MASK = 0 from k on, MASK_PREV from k + 1 on"""
    mask = np.ones((N, len(stops)))
    for b, k in enumerate(stops):
        if k is not None:
            mask[k:, b] = 0.0
    mask_prev = np.ones_like(mask)
    mask_prev[1:] = mask[:-1]
    return mask_prev, mask


def bf16_rne(x):
    """fp32 -> the 16 bits of the bf16 nearest to it, ties to even (finite inputs)"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


# ---- compose (air_write_fwd) -------------------------------------------------------------------------------------------

def _att_for_write(B, seed):
    """att records [N,B,16] (fp32) of a section-0 reference whose heads give the plan full control of (s, x, y)"""
    case, ref = attend_case_and_reference(50, 28, (5, 17, 33), 1, seed=seed, B=B)
    return ref["att"].astype(np.float32), case


def _write_theta64(att, t):
    f = np.float64
    s, x, y = (att[t, :, k].astype(f) for k in (H.ATT_S, H.ATT_X, H.ATT_Y))
    zeros = np.zeros_like(s)
    return np.stack([np.stack([f(1.0) / s, zeros, -x / s], axis=1), np.stack([zeros, f(1.0) / s, -y / s], axis=1)], axis=1)


def running_recon64(att, vrec, C, w, return_taps=False):
    """running_recon :429-439 in float64 from fp32 records: sum over the active steps, in step order, of z_pres * window on
    the canvas (theta_recon :353-356)"""
    f = np.float64
    N, B = att.shape[:2]
    R = np.zeros((B, C * C), f)
    taps = []
    for t in range(N):
        wr, aux = ao.transformer(vrec[t].astype(f).reshape(B, w, w), _write_theta64(att, t), (C, C), return_aux=True)
        active = att[t, :, H.ATT_MASK] != 0
        R = R + np.where(active[:, None], att[t, :, H.ATT_Z].astype(f)[:, None] * wr.reshape(B, C * C), np.zeros_like(R))
        taps.append((aux["x"][active], aux["y"][active]))
    return (R, taps) if return_taps else R


WRITE_TAP_MARGIN = 1e-4


@functools.lru_cache(maxsize=None)
def write_case_and_reference(C, w, Z, seed=0, B=3):
    """(case, fp64 reference), built once per process and shared (read-only); drawn again while a tap coordinate of an
    active step lies within 1e-4 window pixels of a clip edge or more than 1 % of the pixels are within 1e-4 of 0 or 1"""
    for attempt in range(16):
        case = _write_case_once(C, w, Z, seed + 31 * attempt, B)
        ref = write_reference(case)
        if ref["tap"] >= WRITE_TAP_MARGIN and ref["in_band"].mean() <= 0.01:
            return case, ref
    raise AssertionError("no draw meets the margins: change the builder")


def write_case(C, w, Z, seed=0, B=3):
    return write_case_and_reference(C, w, Z, seed, B)[0]


def _write_case_once(C, w, Z, seed, B):
    """fp32 inputs of air_write_fwd at N = 16: att (section-0 records), vrec in (0, 1), ml, images with ink.

    The Bernoulli loss :586-589 is ill-conditioned at its two poles: x * log(r + 1e-9) where r ~ 0 under ink, and
    (1 - x) * log(1 - r + 1e-9) where r ~ 1 over background -- an error of 1e-7 in r moves such a pixel's term by more than
    the whole tolerance of the image's loss.  A comparison there would measure the residue, not the kernel, so the images
    are built from the fp64 running reconstruction R: blobs with ink, a noise floor, and then x = 0 wherever R < 1e-3 and
    x = 1 wherever R > 1 - 1e-3 (the terms at the poles vanish identically; every pixel still runs the same code)."""
    N = N_STEPS
    rng = np.random.RandomState(77 * C + w + 1000 * Z + 100003 * seed)
    att, _ = _att_for_write(B, seed)
    vrec = rng.uniform(0.02, 0.45, (N, B, w * w)).astype(np.float32)
    ml = np.concatenate([rng.standard_normal((N, B, Z)), rng.uniform(-2.0, 1.0, (N, B, Z))], axis=2).astype(np.float32)
    R = running_recon64(att, vrec, C, w)
    blobs, _ = blob_canvases(B, C, 2, seed=seed + 5) if C >= 20 else (np.zeros((B, C * C), np.float32), None)
    images = np.clip(blobs + rng.uniform(0.0, 0.6, (B, C * C)) * (rng.uniform(size=(B, C * C)) < 0.5), 0.0, 1.0)
    images = np.where(R < ILL, 0.0, np.where(R > 1.0 - ILL, 1.0, images)).astype(np.float32)
    return dict(C=C, w=w, Z=Z, N=N, B=B, att=att, vrec=vrec, ml=ml, images=images, dyn=dyn_vector(B))


def write_reference(case):
    """air_model.py:351-366, 409-439, 479-496, 580-593 in float64 on the case's fp32 inputs"""
    f = np.float64
    N, B, C, w, Z = case["N"], case["B"], case["C"], case["w"], case["Z"]
    d = _dyn64(case["dyn"])
    att = case["att"].astype(f)
    R, taps = running_recon64(case["att"], case["vrec"], C, w, return_taps=True)
    ml = case["ml"].astype(f)
    kl_vae = np.stack([ao._gauss_kl(d["VAE_PLV"], ml[t, :, Z:], np.exp(ml[t, :, Z:]), d["VAE_PV"], ml[t, :, :Z], d["VAE_PM"])
                       for t in range(N)])
    L = np.zeros(B, f)
    digits = np.zeros(B, np.int32)
    for t in range(N):                                       # :411-493: z KL under the old mask, the rest under the new one
        mp, mk = att[t, :, H.ATT_MASK_PREV] != 0, att[t, :, H.ATT_MASK] != 0
        L = L + np.where(mp, att[t, :, H.ATT_KL_Z], 0.0)
        L = L + np.where(mk, att[t, :, H.ATT_KL_SCALE], 0.0)
        L = L + np.where(mk, att[t, :, H.ATT_KL_SHIFT], 0.0)
        L = L + np.where(mk, kl_vae[t], 0.0)
        digits = digits + mk.astype(np.int32)
    x = case["images"].astype(f)
    r = np.maximum(np.minimum(R, f(1.0)), f(0.0))
    rec_loss = -np.sum(x * np.log(r + f(ao.EPS)) + (f(1.0) - x) * np.log(f(1.0) - r + f(ao.EPS)), axis=1)
    p1, p0 = r + f(ao.EPS), (f(1.0) - r) + f(ao.EPS)
    passes = (R >= 0.0) & (R <= 1.0)                         # Minimum / Maximum pass their gradient at ties
    d_recon = np.where(passes, -d["GRAD_SCALE"] * (x / p1 - (f(1.0) - x) / p0), 0.0)
    # how far an error dR of the running reconstruction moves d_recon: |d/dr| = gsc * (x / p1^2 + (1 - x) / p0^2)
    d_recon_slope = d["GRAD_SCALE"] * (x / p1 ** 2 + (f(1.0) - x) / p0 ** 2)
    in_band = (np.abs(R) < BAND) | (np.abs(R - 1.0) < BAND)
    tap = min(min(tap_margin(tx, w), tap_margin(ty, w)) for tx, ty in taps if tx.size)
    return dict(R=R, recon=r, kl_vae=kl_vae, run_loss=L, run_digits=digits, rec_loss=rec_loss, loss_item=L + rec_loss,
                d_recon=d_recon, d_recon_slope=d_recon_slope, in_band=in_band, tap=tap,
                active=(att[..., H.ATT_MASK] != 0))
