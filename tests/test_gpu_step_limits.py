"""The attend and compose kernels through all 16 steps the model declares (AIR_MAX_STEPS), at the staging thresholds of their
canvases, against float64 references -- and the whole model at max_steps = 16.

Inputs and references: tests/step_limit_cases.py (the margins that keep every comparison away from a discontinuity of the
step logic are asserted on the CPU by tests/test_step_limit_cases.py).  Everything goes through the C ABI (air._hip)."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import step_limit_cases as slc
from oracle import air_oracle as ao
from oracle import air_oracle_torch as at
from oracle.synth import blob_canvases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


@pytest.fixture(scope="module")
def am(H):
    from air import air_model
    return air_model


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _t(a):
    return torch.tensor(np.ascontiguousarray(a), device="cuda")


def _np(t):
    return t.detach().cpu().numpy()


SENTINEL16 = 0x7FC1          # a bf16 NaN pattern no rounding of a window value produces


def _attend_fwd(H, case, twin=True, expect=0):
    """one air_attend_fwd launch on a case of step_limit_cases; every output starts as NaN / a sentinel"""
    N, B, w = case["N"], case["B"], case["w"]
    d = {k: _t(case[k]) for k in ("hid", "wout", "bout", "canvas", "eps_scale", "eps_shift", "u", "dyn")}
    out7 = torch.full((N, B, H.OUT_STRIDE), float("nan"), device="cuda")
    att = torch.full((N, B, H.ATT_STRIDE), float("nan"), device="cuda")
    window = torch.full((N, B, w * w), float("nan"), device="cuda")
    window16 = torch.full((N, B, w * w), SENTINEL16, dtype=torch.int16, device="cuda")
    Hs, Hh, Hz = case["heads"]
    a = H.AttendFwd(_p(d["hid"]), _p(d["wout"]), _p(d["bout"]), _p(d["canvas"]), _p(d["eps_scale"]), _p(d["eps_shift"]),
                    _p(d["u"]), _p(d["dyn"]), _p(out7), _p(att), _p(window), B, N, case["C"], w, Hs, Hh, Hz,
                    case["wout_ld"], case["train"], _p(window16 if twin else None))
    rc = H.lib().air_attend_fwd(C.byref(a), _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, expect)
    return dict(out7=_np(out7), att=_np(att), window=_np(window), window16=_np(window16).view(np.uint16))


ATT_SCALARS = ("S", "X", "Y", "ZPRE", "Z", "ZPROB")
MEASURED = {}


def _note(key, name, value):
    MEASURED.setdefault(key, {})[name] = max(MEASURED.get(key, {}).get(name, 0.0), float(value))


def _assert_attend(H, case, ref, got, key="attend"):
    """sections 1's assertions on one launch"""
    def close(name, g, r, rel):
        err = float(np.abs(g - r).max())
        _note(key, name, err / max(1.0, float(np.abs(r).max())))
        assert err <= rel * max(1.0, float(np.abs(r).max())), (name, err, float(np.abs(r).max()))

    assert np.isfinite(got["out7"]).all() and np.isfinite(got["att"]).all() and np.isfinite(got["window"]).all()
    close("out7", got["out7"][..., :7], ref["out7"][..., :7], 5e-5)
    assert not got["out7"][..., 7].any()
    for name in ATT_SCALARS:
        k = getattr(H, "ATT_" + name)
        close(name, got["att"][..., k], ref["att"][..., k], 5e-5)
    close("ST_BACK", got["att"][..., H.ATT_ST_BACK:H.ATT_ST_BACK + 3], ref["att"][..., H.ATT_ST_BACK:H.ATT_ST_BACK + 3], 5e-5)
    assert not got["att"][..., H.ATT_ST_BACK + 3].any() and not got["att"][..., H.ATT_KL_VAE].any()
    close("window", got["window"], ref["window"], 5e-5)
    for name in ("KL_Z", "KL_SCALE", "KL_SHIFT"):
        k = getattr(H, "ATT_" + name)
        close(name, got["att"][..., k], ref["att"][..., k], 1e-4)
    mask, mask_prev = got["att"][..., H.ATT_MASK], got["att"][..., H.ATT_MASK_PREV]
    assert np.array_equal(mask, ref["att"][..., H.ATT_MASK]) and np.array_equal(mask_prev, ref["att"][..., H.ATT_MASK_PREV])
    # "a step's z is bit-identical wherever it is recomputed": block (b, t) derives the mask block (b, t - 1) wrote
    assert np.array_equal(mask_prev[1:].view(np.uint32), mask[:-1].view(np.uint32))
    assert (mask_prev[0].view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
    if not case["train"]:
        assert np.array_equal(got["att"][..., H.ATT_Z], ref["att"][..., H.ATT_Z])


@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("Cc,w,heads", slc.ATTEND_CASES)
def test_attend_fwd_sixteen_steps_matches_fp64(H, Cc, w, heads, train):
    """air_attend_fwd at N = 16, B = 4 -- one image alive through all 16 steps, the others stopping at steps 0, 7 and 15 --
    against the float64 restatement of the oracle's step loop (step_limit_cases.attend_reference): the lanes 8 + t' of wave 0
    that recompute the earlier steps' z_pres, the sh_zlo / sh_hprev tables, the `dot < 7 + t` loop up to t = 15, head widths
    from 1 (one lane of a 16-lane group) to 256, canvases on both sides of the C * C <= 2560 staging threshold.
    Bounds: _assert_forward's (tests/test_gpu_configs.py) for the same quantities; masks exact; MASK_PREV[t] == MASK[t - 1]
    bit for bit; the bf16 twin of the window == RNE(window) bit for bit, and a launch without a twin gives the same bits.
    Measured on MI355X (largest over all cases, relative to max(1, |ref|max)): out7 1.2e-07, S 8.5e-08, X 1.6e-07,
    Y 2.0e-07, ZPRE 1.7e-07, Z 1.0e-07, ZPROB 8.5e-08, ST_BACK 2.5e-07, window 1.7e-05, KL_Z 1.9e-07, KL_SCALE 1.7e-07,
    KL_SHIFT 1.5e-07.  The window is the glimpse's amplification of the error of (s, x, y): |grad canvas| * (C - 1.001) / 2
    source pixels per unit of x -- 64 x at C = 128.  With head products that cancel from terms ~50 x their sum (a first
    form of the builder) the same kernel gave x to 1.4e-06 and the window to 8.8e-05 at C = 128; the bound stayed, the
    builder now conditions its products like Glorot weights do (step_limit_cases._attend_case_once)."""
    case, ref = slc.attend_case_and_reference(Cc, w, tuple(heads), train)
    got = _attend_fwd(H, case, twin=True)
    _assert_attend(H, case, ref, got)
    print("attend maxima so far:", {k: "%.1e" % v for k, v in MEASURED["attend"].items()})
    assert np.array_equal(got["window16"], slc.bf16_rne(got["window"]))
    plain = _attend_fwd(H, case, twin=False)
    assert (plain["window16"] == SENTINEL16).all()                  # no twin asked for, none written
    for k in ("out7", "att", "window"):
        assert np.array_equal(plain[k].view(np.uint32), got[k].view(np.uint32)), k


@pytest.mark.parametrize("Cc", [50, 51])
@pytest.mark.parametrize("heads,wide", [((1, 1, 1), 64), ((256, 256, 256), 264)])
def test_attend_fwd_padded_wout_stride_is_bit_identical(H, Cc, heads, wide):
    """wout rows at a stride beyond the widest head (the pad filled with NaN): the kernel stages 7 * wout_ld floats, and the
    launch reserves that much (it reserved 7 * HT: a stride of 64 with one-wide heads ran over sh_hprev / sh_img).  Same bits as
    the tight stride, and still within the bounds of the fp64 reference."""
    case, ref = slc.attend_case_and_reference(Cc, 28, heads, 1)
    tight = _attend_fwd(H, case)
    padded_case = slc.restride_wout(case, wide)
    assert np.isnan(padded_case["wout"][:, max(heads):]).all()
    padded = _attend_fwd(H, padded_case)
    for k in ("out7", "att", "window", "window16"):
        assert np.array_equal(padded[k].view(np.uint16), tight[k].view(np.uint16)), k
    _assert_attend(H, padded_case, ref, padded, key="attend_padded")


def test_wout_stride_below_the_widest_head_is_refused(H):
    """wout_ld < max(Hs, Hh, Hz): AIR_EINVAL from air_attend_fwd, air_attend_bwd and air_heads_out_wgrad, nothing launched
    (every output keeps what it held)"""
    case, ref = slc.attend_case_and_reference(50, 28, (5, 17, 33), 1)
    short = dict(case, wout_ld=32, wout=np.zeros((7, 33), np.float32))
    got = _attend_fwd(H, short, expect=H.EINVAL)
    assert np.isnan(got["out7"]).all() and np.isnan(got["att"]).all() and np.isnan(got["window"]).all()
    assert (got["window16"] == SENTINEL16).all()
    N, B, w, HT = case["N"], case["B"], case["w"], case["HT"]
    d = {k: _t(case[k]) for k in ("hid", "canvas", "eps_scale", "eps_shift", "dyn")}
    wout = torch.zeros(7, 33, device="cuda")
    out7, att = _t(ref["out7"].astype(np.float32)), _t(ref["att"].astype(np.float32))
    d_win, d_sxy = torch.zeros(N, B, w * w, device="cuda"), torch.zeros(N, B, 4, device="cuda")
    d_hid, d_out7 = torch.full((N, B, HT), 7.0, device="cuda"), torch.full((N, B, H.OUT_STRIDE), 7.0, device="cuda")
    ab = H.AttendBwd(_p(d["hid"]), _p(wout), _p(d["canvas"]), _p(d["eps_scale"]), _p(d["eps_shift"]), _p(d["dyn"]), _p(out7),
                     _p(att), _p(d_win), _p(d_sxy), _p(d_hid), _p(d_out7), B, N, 50, w, 5, 17, 33, 32, 0)
    assert H.lib().air_attend_bwd(C.byref(ab), _stream()) == H.EINVAL
    dwout, dbout = torch.full((7, 33), 7.0, device="cuda"), torch.full((7,), 7.0, device="cuda")
    assert H.lib().air_heads_out_wgrad(_p(d_out7), _p(d["hid"]), _p(dwout), _p(dbout), N * B, 5, 17, 33, 32, _stream()) == H.EINVAL
    torch.cuda.synchronize()
    for t in (d_hid, d_out7, dwout, dbout):
        assert bool((t == 7.0).all())
    # the widest head itself is enough
    ab.wout_ld = 33
    assert H.lib().air_attend_bwd(C.byref(ab), _stream()) == 0
    assert H.lib().air_heads_out_wgrad(_p(d_out7), _p(d["hid"]), _p(dwout), _p(dbout), N * B, 5, 17, 33, 33, _stream()) == 0
    torch.cuda.synchronize()


# ---- compose ---------------------------------------------------------------------------------------------------------------

D_R = 2e-5       # the bound on the reconstruction itself, carried through d loss / d r below


@pytest.mark.parametrize("Cc,w,Z", slc.WRITE_CASES)
def test_write_fwd_sixteen_steps_matches_fp64(H, Cc, w, Z):
    """air_write_fwd at N = 16, B = 3 (images alive for 16, 7 and 15 steps) on the att records of the section-0 reference:
    compose_pixel over up to 16 live steps, the `tid < N` record fetch and thread 0's running-loss loop, the per-wave VAE-KL
    loop at Z = 1, 50, 65 (> one wave), 130, canvases on both sides of the C * C <= 4096 image-prefetch threshold.
    reconstruction <= 2e-5; digit counts exact; KL_VAE of every step, the inactive ones included, <= 1e-4 of max(1, |ref|max)
    (the bound of the other KLs); the three losses rtol 1e-5 / atol 1e-3; wb_order a permutation with every inactive item
    behind every active one.
    d_recon = pass ? -gsc * (x / (r + 1e-9) - (1 - x) / (1 - r + 1e-9)) : 0 at every pixel whose fp64 running reconstruction is
    >= 1e-4 away from 0 and 1 (at most 1 % are not: asserted on the CPU): exactly 0 where the clip does not pass, else within
    what an error of 2e-5 in r -- the bound on the reconstruction -- moves the formula by, + 1e-6 relative for the fp32
    division and products.
    Measured on MI355X (largest over the cases): reconstruction 8.4e-06, KL_VAE 8.4e-08 relative, run_loss 1.6e-07 /
    rec_loss 7.9e-07 / loss_item 7.0e-07 relative, d_recon error 0.41 of its allowance."""
    case, ref = slc.write_case_and_reference(Cc, w, Z)
    N, B = case["N"], case["B"]
    att_in = case["att"].copy()
    att_in[..., H.ATT_KL_VAE] = np.nan
    vrec, ml, images, dyn, att = (_t(v) for v in (case["vrec"], case["ml"], case["images"], case["dyn"], att_in))
    recon, d_recon = torch.full((B, Cc * Cc), float("nan"), device="cuda"), torch.full((B, Cc * Cc), float("nan"), device="cuda")
    rec_loss, run_loss, loss_item = (torch.full((B,), float("nan"), device="cuda") for _ in range(3))
    digits = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    order = torch.full((N * B,), -1, dtype=torch.int32, device="cuda")
    wf = H.WriteFwd(_p(vrec), _p(ml), _p(images), _p(dyn), _p(att), _p(recon), _p(rec_loss), _p(d_recon), _p(run_loss),
                    _p(digits), _p(loss_item), B, N, Cc, w, Z, _p(order))
    H.check(H.lib().air_write_fwd(C.byref(wf), _stream()), "air_write_fwd")
    torch.cuda.synchronize()
    recon, d_recon, att_out, order = _np(recon), _np(d_recon), _np(att), _np(order)
    err = float(np.abs(recon - ref["recon"]).max())
    print("|d recon| %.2e" % err)
    assert err <= 2e-5
    assert np.array_equal(_np(digits), ref["run_digits"])
    kl = att_out[..., H.ATT_KL_VAE]
    kl_err = float(np.abs(kl - ref["kl_vae"]).max()) / max(1.0, float(np.abs(ref["kl_vae"]).max()))
    print("KL_VAE %.2e of %.1f" % (kl_err, np.abs(ref["kl_vae"]).max()))
    assert np.isfinite(kl).all() and kl_err <= 1e-4
    keep = [k for k in range(H.ATT_STRIDE) if k != H.ATT_KL_VAE]
    assert np.array_equal(att_out[..., keep], case["att"][..., keep])          # the records are read, not rewritten
    for name, got in (("run_loss", run_loss), ("rec_loss", rec_loss), ("loss_item", loss_item)):
        print("%s: relative error %.2e" % (name, float(np.abs(_np(got) - ref[name]).max() / np.abs(ref[name]).max())))
        np.testing.assert_allclose(_np(got), ref[name], rtol=1e-5, atol=1e-3, err_msg=name)
    # d_recon
    f = np.float64
    cmp = ~ref["in_band"]
    x, r, gsc = case["images"].astype(f), ref["recon"], f(case["dyn"][H.DYN_GRAD_SCALE])
    p1, p0 = r + ao.EPS, (1.0 - r) + ao.EPS
    passes = (ref["R"] >= 0.0) & (ref["R"] <= 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        allow = gsc * (x * (1.0 / (p1 - D_R) - 1.0 / p1) + (1.0 - x) * (1.0 / (p0 - D_R) - 1.0 / p0)) + 1e-6 * np.abs(ref["d_recon"])
    sel = cmp & passes
    assert sel.mean() >= 0.3 and (cmp & ~passes).mean() >= 0.02
    assert not d_recon[cmp & ~passes].any()
    derr = np.abs(d_recon - ref["d_recon"])
    print("d_recon: worst error / allowance %.2e over %d pixels" % (float((derr[sel] / np.maximum(allow[sel], 1e-300)).max()), int(sel.sum())))
    assert (derr[sel] <= allow[sel]).all()
    # the longest-first list of the write backward
    assert np.array_equal(np.sort(order), np.arange(N * B))
    active = ref["active"].reshape(-1)[order]                                 # item = t * B + b
    n_act = int(ref["active"].sum())
    assert active[:n_act].all() and not active[n_act:].any()


# ---- attend backward ---------------------------------------------------------------------------------------------------------

def _attend_loss_torch(H_, case, d_window, d_sxy, mask, mask_prev):
    """float64 torch twin of section 1's forward, reduced to the scalar whose gradient air_attend_bwd computes:
    <d_window, window> + <d_sxy_write, (s, x, y, z)> + grad_scale * sum(mask * (KL scale + KL shift) + mask_prev * KL z)"""
    f64 = torch.float64
    N, B, Cc, w = case["N"], case["B"], case["C"], case["w"]
    dv = lambda k: float(case["dyn"][k])  # noqa: E731
    hid = torch.tensor(case["hid"], dtype=f64, requires_grad=True)
    wout, bout = torch.tensor(np.nan_to_num(case["wout"]), dtype=f64), torch.tensor(case["bout"], dtype=f64)
    cols = [hid[..., off:off + wid] @ wout[o, :wid] + bout[o] for o, (off, wid) in enumerate(slc.head_layout(*case["heads"]))]
    out7 = torch.stack(cols, dim=-1)
    out7.retain_grad()
    canvas = torch.tensor(case["canvas"], dtype=f64).reshape(B, Cc, Cc)
    T, plo, gsc = dv(H_.DYN_TEMPERATURE), dv(H_.DYN_PRIOR_LOG_ODDS), dv(H_.DYN_GRAD_SCALE)
    total = torch.zeros((), dtype=f64)
    tt = lambda a: torch.tensor(a, dtype=f64)  # noqa: E731
    for t in range(N):
        o = out7[t]
        s = torch.sigmoid(o[:, 0] + tt(case["eps_scale"][t, :, 0]) * torch.sqrt(torch.exp(o[:, 1])))
        xy = torch.tanh(o[:, 2:4] + tt(case["eps_shift"][t]) * torch.sqrt(torch.exp(o[:, 4:6])))
        zeros = torch.zeros_like(s)
        theta = torch.stack([torch.stack([s, zeros, xy[:, 0]], 1), torch.stack([zeros, s, xy[:, 1]], 1)], 1)
        window = at.transformer(canvas, theta, (w, w)).reshape(B, w * w)
        u = tt(case["u"][t])
        z_pre = (o[:, 6] + torch.log(u + ao.EPS) - torch.log(1.0 - u + ao.EPS)) / T
        z = torch.sigmoid(z_pre)
        kl_z = at._concrete_kl(z_pre, plo, T, o[:, 6], T)
        kl_s = at._gauss_kl(dv(H_.DYN_SCALE_PLV), o[:, 1:2], torch.exp(o[:, 1:2]), dv(H_.DYN_SCALE_PV), o[:, 0:1], dv(H_.DYN_SCALE_PM))
        kl_h = at._gauss_kl(dv(H_.DYN_SHIFT_PLV), o[:, 4:6], torch.exp(o[:, 4:6]), dv(H_.DYN_SHIFT_PV), o[:, 2:4], dv(H_.DYN_SHIFT_PM))
        sxyz = torch.stack([s, xy[:, 0], xy[:, 1], z], 1)
        total = total + (tt(d_window[t]) * window).sum() + (tt(d_sxy[t]) * sxyz).sum()
        total = total + gsc * (tt(mask[t]) * (kl_s + kl_h) + tt(mask_prev[t]) * kl_z).sum()
    total.backward()
    return out7.grad.numpy(), (hid.grad * (hid.detach() > 0)).numpy()


@pytest.mark.parametrize("Cc", [50, 51])
def test_attend_bwd_exact_adjoint_sixteen_steps_matches_autograd(H, Cc):
    """air_attend_bwd(literal = 0) at N = 16, B = 3 (alive for 16, 7 and 15 steps), staged (C = 50) and unstaged (51) canvas,
    against torch autograd in float64 through a twin of section 1's forward.  The gradients that arrive from the write path
    and the VAE (d_sxy_write, d_window) are zero for an inactive item, as air_write_bwd leaves them.
    d_out7 per (step, unit) within 1e-4 of the largest reference element of that step, the bound of
    test_attend_bwd_graph_order_read_gradient_matches_oracle; d_hid per (step, head segment) likewise; d_hid exactly 0 where
    MASK_PREV == 0; the wout pad (NaN) and a padded stride change no bit.
    Measured on MI355X: d_out7 2.6e-05, d_hid 2.6e-05 of those scales."""
    heads = (5, 17, 33)
    case, ref = slc.attend_case_and_reference(Cc, 28, heads, 1, B=3)
    N, B, w, HT = case["N"], case["B"], case["w"], case["HT"]
    mask, mask_prev = ref["att"][..., H.ATT_MASK], ref["att"][..., H.ATT_MASK_PREV]
    assert (mask_prev == 0).sum() >= 8 and (mask != mask_prev).sum() == 2
    rng = np.random.RandomState(Cc)
    d_window = (rng.standard_normal((N, B, w * w)) * mask[..., None]).astype(np.float32)
    d_sxy = (rng.standard_normal((N, B, 4)) * mask[..., None]).astype(np.float32)
    want7, want_hid = _attend_loss_torch(H, case, d_window, d_sxy, mask, mask_prev)

    def run(c):
        d = {k: _t(c[k]) for k in ("hid", "wout", "canvas", "eps_scale", "eps_shift", "dyn")}
        out7, att = _t(ref["out7"].astype(np.float32)), _t(ref["att"].astype(np.float32))
        dw, ds = _t(d_window), _t(d_sxy)
        d_hid = torch.full((N, B, HT), float("nan"), device="cuda")
        d_out7 = torch.full((N, B, H.OUT_STRIDE), float("nan"), device="cuda")
        ab = H.AttendBwd(_p(d["hid"]), _p(d["wout"]), _p(d["canvas"]), _p(d["eps_scale"]), _p(d["eps_shift"]), _p(d["dyn"]),
                         _p(out7), _p(att), _p(dw), _p(ds), _p(d_hid), _p(d_out7), B, N, Cc, w, *heads, c["wout_ld"], 0)
        H.check(H.lib().air_attend_bwd(C.byref(ab), _stream()), "air_attend_bwd")
        torch.cuda.synchronize()
        return _np(d_out7), _np(d_hid)

    got7, got_hid = run(case)
    assert np.isfinite(got7).all() and np.isfinite(got_hid).all() and not got7[..., 7].any()
    worst7 = worst_h = 0.0
    segs = sorted(set(slc.head_layout(*heads)))
    for t in range(N):
        for k in range(7):
            scale = max(np.abs(want7[t, :, k]).max(), 1e-6)
            e = np.abs(got7[t, :, k] - want7[t, :, k]).max() / scale
            worst7 = max(worst7, e)
            assert e <= 1e-4, (t, k, got7[t, :, k], want7[t, :, k])
        for off, wid in segs:
            scale = max(np.abs(want_hid[t, :, off:off + wid]).max(), 1e-6)
            e = np.abs(got_hid[t, :, off:off + wid] - want_hid[t, :, off:off + wid]).max() / scale
            worst_h = max(worst_h, e)
            assert e <= 1e-4, (t, off, e)
    print("attend_bwd N = 16: d_out7 %.2e, d_hid %.2e of the per-step scales" % (worst7, worst_h))
    assert not got_hid[mask_prev == 0].any() and not got7[mask_prev == 0].any()
    assert got_hid[(mask_prev == 1) & (mask == 0)].any()                    # the stopping step still has its z KL
    wide7, wide_hid = run(slc.restride_wout(case, 40))
    assert np.array_equal(wide7.view(np.uint32), got7.view(np.uint32))
    assert np.array_equal(wide_hid.view(np.uint32), got_hid.view(np.uint32))


# ---- the whole model at its declared limits ----------------------------------------------------------------------------------

LIMIT_HP = dict(ao.TRAINING_HP, max_steps=16, windows_size=32, canvas_size=50, max_digits=2)


def _limit_model(am, images, targets, params, noise, train=True, backward="exact"):
    am.reset_default_graph()
    m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"),
                    cnn=False, train=train, scope="air", gemm_precision="fp32", backward=backward, **LIMIT_HP)
    m.load_state_dict(params)
    m.set_noise(noise)
    m.set_dynamic(z_pres_prior_log_odds=-2.0)
    return m


def test_model_at_sixteen_steps_and_the_largest_window(am):
    """AIRModel(max_steps = 16, windows_size = 32, canvas_size = 50), B = 2, with the z_pres output bias raised so that the
    images stay alive (asserted on the oracle first: one of them for >= 12 steps): forward parity with _assert_forward's
    bounds, fp32 gradients of the exact adjoint against the fp64 graph with test_ragged_configurations' bounds, and one
    training() step each with backward = "reference" and "reference_carried": variables finite, and moved if and only if
    they had a gradient."""
    from test_gpu_configs import _assert_forward
    hp, B = LIMIT_HP, 2
    images, targets = blob_canvases(B, hp["canvas_size"], hp["max_digits"], seed=11)
    params, noise = ao.init_params(hp, 3), ao.make_noise(hp, B, 8)
    params["z_pres/log_odds/output/biases"] = np.full(1, 7.0, np.float32)
    o = ao.air_forward(params, images, targets, noise, hp, True, -2.0, early_exit=True)
    print("oracle: steps executed %d, digits %s" % (o["steps_executed"], o["rec_num_digits"].tolist()))
    assert o["rec_num_digits"].max() >= 12
    m = _limit_model(am, images, targets, params, noise)
    m.forward()
    assert m.steps_executed == o["steps_executed"]
    _assert_forward(m, o, images)
    assert abs(float(m.loss) - float(o["loss"])) / abs(float(o["loss"])) <= 1e-2
    s = m._stream()
    m._run_forward(s)
    m._run_backward(s)
    torch.cuda.synchronize()
    f64 = torch.float64
    pt = at.to_torch(params, dtype=f64, requires_grad=True)
    _, grads = at.loss_and_grads(pt, torch.tensor(images, dtype=f64), torch.tensor(targets), at.to_torch(noise, dtype=f64), hp, -2.0)
    worst = {}
    for k, gref in grads.items():
        got = m.gradients[k].detach().cpu().double()
        err = float((got - gref).norm() / (gref.norm() + 1e-30))
        where = k.startswith(("z_pres", "scale", "shift"))
        worst[where] = max(worst.get(where, 0.0), err)
        assert err <= (0.25 if where else 5e-2), (k, err)
    print("N = 16 gradients, worst relative L2: where-heads %.2e, others %.2e" % (worst[True], worst[False]))
    for backward in ("reference", "reference_carried"):
        m = _limit_model(am, images, targets, params, noise, backward=backward)
        s = m._stream()
        m._run_forward(s)
        m._run_backward(s)
        torch.cuda.synchronize()
        has_grad = {k: bool(v.abs().max() > 0) for k, v in m.gradients.items()}
        before = {k: _np(v).copy() for k, v in m.variables.items()}
        m.training()
        torch.cuda.synchronize()
        assert np.isfinite(float(m.loss)) and int(m.global_step) == 1
        for k, v in m.variables.items():
            a = _np(v)
            assert np.all(np.isfinite(a)), (backward, k)
            assert np.array_equal(a, before[k]) == (not has_grad[k]), (backward, k)


def test_constructor_refuses_shapes_whose_launches_exceed_the_lds(am):
    """The taps and windows of all steps of an image live in the LDS of one compose workgroup: (16 + 7 * 16 + N * (8 * C +
    w * w)) * 4 bytes -- at max_steps = 16, windows_size = 32 more than the 160 KB of a workgroup from canvas_size = 192 on.
    The constructor says so (NotImplementedError naming canvas_size and max_steps) instead of the first forward failing
    inside air_write_fwd; the same canvas with max_steps = 3 constructs and runs.
    What a launch did above the limit before: air_grant_lds (csrc/air_common.h), which every sampler entry point calls
    through ensure_lds before its launch, returns AIR_ELIMIT for bytes > 160 * 1024 as its first statement -- before any
    driver call and before hipLaunchKernelGGL.  So the ABI never launched an over-sized workgroup: the caller got error
    code -2 from air_write_fwd, which AIRModel turned into an AirHipError in the middle of forward()."""
    B = 2
    kw = dict(ao.TRAINING_HP, windows_size=32, canvas_size=200)
    images = torch.zeros(B, 200 * 200, device="cuda")
    targets = torch.zeros(B, dtype=torch.int32, device="cuda")
    am.reset_default_graph()
    with pytest.raises(NotImplementedError, match=r"canvas_size.*max_steps"):
        am.AIRModel(images, targets, cnn=False, train=False, scope="air", gemm_precision="fp32", **dict(kw, max_steps=16))
    # a train model at this canvas is refused at any step count: the write backward keeps the whole canvas in LDS
    am.reset_default_graph()
    with pytest.raises(NotImplementedError, match=r"air_write_bwd"):
        am.AIRModel(images, targets, cnn=False, train=True, scope="air", gemm_precision="fp32", **dict(kw, max_steps=3))
    am.reset_default_graph()
    img, _ = blob_canvases(B, 200, 2, seed=4)
    m = am.AIRModel(torch.tensor(img, device="cuda"), targets, cnn=False, train=False, scope="air", gemm_precision="fp32",
                    **dict(kw, max_steps=3))
    m.forward()
    torch.cuda.synchronize()
    rec = _np(m.reconstruction)
    assert 1 <= m.steps_executed <= 3 and np.isfinite(float(m.loss))
    assert np.isfinite(rec).all() and rec.min() >= 0.0 and rec.max() <= 1.0
