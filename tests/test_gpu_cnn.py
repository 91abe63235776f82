"""GPU tests of air.cnn and the air_cnn_* entry points (the CNN front-end of the reference's air_model.py:510-533 as a
differentiable op on its own HIP kernels).

The reference arithmetic is a float64 torch-CPU restatement written here (_reference): F.conv2d(padding=2), clamp(min=0),
F.max_pool2d(2, 2) on NCHW permutations of the NHWC tensors -- no executed graph of the reference holds this block.

PRECONDITION of every comparison, asserted on the float64 reference alone: the smallest |pre-activation| of the three
layers and the smallest gap between the two largest values of a pool window with a positive maximum are >= 1e-5, so fp32
and float64 route every gradient through the same ReLU branch and the same window element.  It is a condition on the
inputs, not a tolerance; no element is ever excluded from a comparison.

  * routing, exactly, through the C ABI: arg1 / arg2 are the reference's first-max codes, pool1 > 0, pool2 > 0, out > 0 its masks;
  * the first-max tie rule alone: an all-zero image makes every conv1 pre-activation its bias, so every arg1 code is 0;
  * forward and gradients (of sum(w * out), all six variables and d_images) against float64, each relative to its tensor's
    max |reference|.  Measured on the MI355X (worst over the six cases below): MEASURED_FWD, MEASURED_GRAD; asserted:
    4 x measured (room for another accumulation order after a re-tiling), capped at 1e-4 -- exact fp32 products of
    K <= 200 per layer, three layers deep, cannot be further, so anything beyond the cap is a bug;
  * the inference forward (torch.no_grad(), or the ABI without the saved tensors) and both input forms: the same bits;
  * d_images only when the input requires a gradient, the variable gradients unchanged bit for bit;
  * determinism at B = 70 and the variables round trip.
Stream capture is not tested: the op refuses it (air/cnn.py), like air.vae."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from oracle.synth import blob_canvases

pytestmark = pytest.mark.gpu

f32 = np.float32
# (seed, B, S, F): the reference's own size; odd 13 -> 6 -> 3 (a dropped row, then an odd plane); F < 8 on a 4 x 4 plane where
# every pixel sees padding; the halo covers the whole image, 5 -> 2 -> 1; even sizes throughout with F = 5; the batch
# reduction and the grid at B = 70.  The last case is the S = 9, F = 3 recipe again; its seed is the first from 2 upward at
# which the float64 reference meets the precondition at B = 70 (ReLU margin at seeds 2..5: 8.6e-7, 1.1e-5 with a pool
# margin of 7.2e-6, 1.4e-5 with 9.8e-6, 2.6e-7; seed 6: 1.1e-5 and 1.7e-4)
CASES = [(1, 2, 50, 8), (2, 3, 13, 8), (2, 2, 9, 3), (3, 1, 5, 8), (5, 2, 28, 5), (6, 70, 9, 3)]
MARGIN = 1e-5
# worst |value - reference| / max |reference| measured on the MI355X (printed by the tests below)
#   forward: 7.05e-07 (out, the blob canvases; the six cases lie between 1.5e-07 and 6.2e-07, worst tensor each)
#   gradients: 8.03e-07 (cnn/conv1/kernel, B = 2, S = 50, F = 8; the six cases lie between 1.6e-07 and 8.03e-07)
MEASURED_FWD = 7.05e-7
MEASURED_GRAD = 8.03e-7
FWD_BOUND = min(4 * MEASURED_FWD, 1e-4)
GRAD_BOUND = min(4 * MEASURED_GRAD, 1e-4)
NAMES = ["cnn/conv%d/%s" % (i, kind) for i in (1, 2, 3) for kind in ("kernel", "bias")]


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import cnn
    return cnn


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.detach().contiguous().view(torch.int32), b.detach().contiguous().view(torch.int32))


def _variables(seed, F):
    rng = np.random.RandomState(seed)
    c = 1
    P = {}
    for i in (1, 2, 3):
        lim = np.sqrt(6.0 / (25 * c + 25 * F))
        P["cnn/conv%d/kernel" % i] = rng.uniform(-lim, lim, (5, 5, c, F)).astype(f32)
        P["cnn/conv%d/bias" % i] = rng.uniform(-0.1, 0.1, F).astype(f32)
        c = F
    return P


def _codes(idx, width):
    """flat indices of F.max_pool2d into the [H, W] plane -> 2 dy + dx of the 2x2 window, NHWC"""
    n = idx.shape[-1]
    wy = torch.arange(n).view(1, 1, n, 1)
    wx = torch.arange(n).view(1, 1, 1, n)
    code = 2 * (idx // width - 2 * wy) + (idx % width - 2 * wx)
    assert int(code.min()) >= 0 and int(code.max()) <= 3
    return code.permute(0, 2, 3, 1).contiguous().numpy().astype(np.uint8)


def _pool_margin(r):
    """smallest gap between the two largest values of a 2x2 window whose maximum is positive"""
    B, F_, H, W = r.shape
    n = H // 2
    if n == 0:
        return float("inf")
    win = r[:, :, :2 * n, :2 * n].reshape(B, F_, n, 2, n, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
    top = torch.sort(win, dim=1, descending=True).values
    live = top[:, 0] > 0
    return float((top[live, 0] - top[live, 1]).min()) if bool(live.any()) else float("inf")


def _reference(P, images_nchw, w):
    """float64: every tensor the kernels produce (NHWC), the routing, the margins, and the gradients of sum(w * out)"""
    x = torch.tensor(images_nchw, dtype=torch.float64, requires_grad=True)
    V = [torch.tensor(P[n], dtype=torch.float64, requires_grad=True) for n in NAMES]
    conv = lambda h, k, b: TF.conv2d(h, k.permute(3, 2, 0, 1), b, padding=2)  # noqa: E731
    pre1 = conv(x, V[0], V[1]); r1 = pre1.clamp(min=0.0); p1, i1 = TF.max_pool2d(r1, 2, 2, return_indices=True)
    pre2 = conv(p1, V[2], V[3]); r2 = pre2.clamp(min=0.0); p2, i2 = TF.max_pool2d(r2, 2, 2, return_indices=True)
    pre3 = conv(p2, V[4], V[5]); r3 = pre3.clamp(min=0.0)
    out = r3.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    ref = dict(out=out.detach().numpy(), pool1=p1.detach().permute(0, 2, 3, 1).contiguous().numpy(),
               pool2=p2.detach().permute(0, 2, 3, 1).contiguous().numpy(),
               arg1=_codes(i1, r1.shape[-1]), arg2=_codes(i2, r2.shape[-1]),
               relu_margin=min(float(t.detach().abs().min()) for t in (pre1, pre2, pre3)),
               pool_margin=min(_pool_margin(r1.detach()), _pool_margin(r2.detach())))
    if w is not None:
        grads = torch.autograd.grad((out * torch.tensor(w, dtype=torch.float64)).sum(), [x] + V)
        ref["d_images"] = grads[0].numpy().reshape(x.shape[0], -1)
        for n, g in zip(NAMES, grads[1:]):
            ref[n] = g.numpy()
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _case(seed, B, S, F):
    """(variables, images [B, S*S] fp32, w, reference); computed once, read-only"""
    P = _variables(seed, F)
    images = np.random.RandomState(1000 + seed).uniform(0, 1, (B, 1, S, S)).astype(f32)
    w = np.random.RandomState(2000 + seed).randn(B, (S // 4) ** 2 * F)
    ref = _reference(P, images, w)
    flat = images.reshape(B, S * S)
    for a in list(P.values()) + [flat, w]:
        a.setflags(write=False)
    # the precondition, on the float64 reference alone
    assert ref["relu_margin"] >= MARGIN and ref["pool_margin"] >= MARGIN, (ref["relu_margin"], ref["pool_margin"])
    return P, flat, w, ref


def _dev(a):
    return torch.tensor(np.asarray(a), device="cuda")


def _module(M, P, S, F):
    m = M.CNN(S, F, device="cuda")
    m.load_variables(P)
    return m


def _abi_forward(P, images, S, F, save):
    """air_cnn_fwd through ctypes: (out, pool1, pool2, arg1, arg2), the last four None without `save`"""
    from air import _hip as H
    B, S1, S2 = images.shape[0], S // 2, S // 4
    x = _dev(images)
    V = [_dev(P[n]) for n in NAMES]
    out = torch.full((B, S2 * S2 * F), float("nan"), device="cuda")
    saved = [None] * 4
    if save:
        saved = [torch.full((B, S1, S1, F), float("nan"), device="cuda"), torch.full((B, S2, S2, F), float("nan"), device="cuda"),
                 torch.full((B, S1, S1, F), 255, dtype=torch.uint8, device="cuda"),
                 torch.full((B, S2, S2, F), 255, dtype=torch.uint8, device="cuda")]
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    a = H.CnnFwd(*[p(t) for t in [x] + V + [out] + saved], B, S, F)
    H.check(H.lib().air_cnn_fwd(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "air_cnn_fwd")
    torch.cuda.synchronize()
    return [out] + saved


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d-B%d-S%d-F%d" % c)
def test_routing_is_exact_through_the_abi(M, case):
    seed, B, S, F = case
    P, images, w, ref = _case(*case)
    out, pool1, pool2, arg1, arg2 = _abi_forward(P, images, S, F, save=True)
    assert np.array_equal(arg1.cpu().numpy(), ref["arg1"])
    assert np.array_equal(arg2.cpu().numpy(), ref["arg2"])
    assert np.array_equal(pool1.cpu().numpy() > 0, ref["pool1"] > 0)
    assert np.array_equal(pool2.cpu().numpy() > 0, ref["pool2"] > 0)
    assert np.array_equal(out.cpu().numpy() > 0, ref["out"] > 0)


def test_first_maximum_wins_a_tie(M):
    seed, B, S, F = CASES[0]
    P = _variables(seed, F)
    out, pool1, pool2, arg1, arg2 = _abi_forward(P, np.zeros((B, S * S), f32), S, F, save=True)
    assert int(arg1.max()) == 0                                     # four equal values: the first one
    b1 = np.maximum(P["cnn/conv1/bias"], 0.0)
    assert np.array_equal(pool1.cpu().numpy(), np.broadcast_to(b1, (B, S // 2, S // 2, F)))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d-B%d-S%d-F%d" % c)
def test_forward_against_float64(M, case):
    seed, B, S, F = case
    P, images, w, ref = _case(*case)
    out, pool1, pool2, _, _ = _abi_forward(P, images, S, F, save=True)
    errs = dict(out=_rel(out.cpu().numpy(), ref["out"]), pool1=_rel(pool1.cpu().numpy(), ref["pool1"]),
                pool2=_rel(pool2.cpu().numpy(), ref["pool2"]))
    print("cnn forward %r: %s" % (case, {k: "%.3g" % v for k, v in errs.items()}))
    assert max(errs.values()) <= FWD_BOUND, errs


def test_forward_on_blob_canvases(M):
    """a multi-MNIST-like canvas (blank regions included: only the forward is compared, it is continuous across a flip)"""
    P = _variables(1, 8)
    images, counts = blob_canvases(4, canvas=50, max_digits=2, seed=7)
    images = np.asarray(images, f32).reshape(4, 2500)
    assert counts.max() > 0 and images.max() > 0
    ref = _reference(P, images.reshape(4, 1, 50, 50), None)
    out, pool1, pool2, _, _ = _abi_forward(P, images, 50, 8, save=True)
    errs = dict(out=_rel(out.cpu().numpy(), ref["out"]), pool1=_rel(pool1.cpu().numpy(), ref["pool1"]),
                pool2=_rel(pool2.cpu().numpy(), ref["pool2"]))
    print("cnn forward blob canvases: %s" % {k: "%.3g" % v for k, v in errs.items()})
    assert max(errs.values()) <= FWD_BOUND, errs


def _run(M, case, images_need_grad=True, module=None):
    """one eager forward + backward of sum(w * out): (module, out, d_images or None, {name: gradient})"""
    seed, B, S, F = case
    P, images, w, ref = _case(*case)
    m = module or _module(M, P, S, F)
    for q in m.parameters():
        q.grad = None
    x = _dev(images).requires_grad_(images_need_grad)
    out = m(x)
    (out * _dev(w.astype(f32))).sum().backward()
    torch.cuda.synchronize()
    return m, out.detach(), x.grad, {n: q.grad.detach().clone() for n, q in zip(NAMES, m._params())}


@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d-B%d-S%d-F%d" % c)
def test_gradients_against_float64(M, case):
    P, images, w, ref = _case(*case)
    m, out, d_images, grads = _run(M, case)
    errs = {n: _rel(g.cpu().numpy(), ref[n]) for n, g in grads.items()}
    errs["d_images"] = _rel(d_images.cpu().numpy(), ref["d_images"])
    print("cnn gradients %r: %s" % (case, {k: "%.3g" % v for k, v in errs.items()}))
    assert max(errs.values()) <= GRAD_BOUND, errs
    assert _rel(out.cpu().numpy(), ref["out"]) <= FWD_BOUND


@pytest.mark.parametrize("case", [CASES[0], CASES[1]], ids=lambda c: "seed%d-B%d-S%d-F%d" % c)
def test_inference_forward_has_the_training_bits(M, case):
    seed, B, S, F = case
    P, images, w, ref = _case(*case)
    m = _module(M, P, S, F)
    x = _dev(images)
    train = m(x)
    assert train.requires_grad
    with torch.no_grad():
        infer = m(x)
        nhwc = m(x.view(B, S, S, 1))
    assert not infer.requires_grad and _same_bits(train, infer) and _same_bits(train, nhwc)
    assert _same_bits(train, m(x.view(B, S, S, 1)))
    assert _same_bits(train, M.cnn(x, S, F, module=m))
    saved = _abi_forward(P, images, S, F, save=True)[0]
    bare = _abi_forward(P, images, S, F, save=False)[0]
    assert _same_bits(saved, bare) and _same_bits(saved, train)
    assert tuple(train.shape) == (B, m.output_dim)


def test_d_images_only_when_asked_for(M):
    case = CASES[1]
    m, out, d_images, grads = _run(M, case, images_need_grad=True)
    m2, out2, none, grads2 = _run(M, case, images_need_grad=False)
    assert d_images is not None and none is None
    assert _same_bits(out, out2)
    for n in NAMES:
        assert _same_bits(grads[n], grads2[n]), n
    # and in the [B, S, S, 1] form the gradient comes back in that shape
    seed, B, S, F = case
    x = _dev(_case(*case)[1]).view(B, S, S, 1).requires_grad_(True)
    m(x).sum().backward()
    assert tuple(x.grad.shape) == (B, S, S, 1)


def test_two_runs_give_the_same_bits(M):
    case = CASES[5]
    assert case[1] == 70
    m, out, d_images, grads = _run(M, case)
    m, out2, d_images2, grads2 = _run(M, case, module=m)
    assert _same_bits(out, out2) and _same_bits(d_images, d_images2)
    for n in NAMES:
        assert _same_bits(grads[n], grads2[n]), n


def test_variables_round_trip(M):
    a = M.CNN(13, 8, device="cuda", seed=5)
    b = M.CNN(13, 8, device="cuda", seed=6)
    x = _dev(_case(*CASES[1])[1])
    with torch.no_grad():
        assert not _same_bits(a(x), b(x))
        b.load_variables(a.variables())
        assert _same_bits(a(x), b(x))
