"""air_cnn_fwd, air_cnn_bwd and air_cnn_bwd_sq at every filter count, at the last canvas of every filter count, on both sides
of every choice of their LDS layout, at the smallest planes and at the edges of their thread counts -- through the C ABI
(ctypes) on guarded buffers, against the float64 restatement of tests/cnn_edge_cases.py (whose conditions
tests/test_cnn_edge_cases.py asserts on the CPU).

Every launch of a case runs once and is shared by the tests (lru_cache).  A case's launches:
  fwd        air_cnn_fwd with the four saved tensors          bwd        air_cnn_bwd on fwd's own saved tensors
  fwd_tails  the same, every input followed by NaNs           bwd_tails  the same, every input followed by NaN / 0xFF
                                                              sq         air_cnn_bwd_sq on the same inputs
Every output lies in an allocation with one extra row of sentinels (7.0, 0xA5) before and after it and starts as NaN
(0xFF for the codes); the workspace is EXACTLY air_cnn_workspace_floats(B, S, F) floats of NaN, sq_partials exactly
air_cnn_num_sq_partials(F): a read before a write, an unwritten partial or an element too few surfaces as a NaN or a dead
sentinel.

  * exact-integer cases: byte equality with the float64 reference cast to fp32 -- out, pool1, pool2, the codes, d_images,
    the six gradients, the per-image partials in the workspace; ties and exact zeros included;
  * real-valued cases: tests/test_gpu_cnn.py's FWD_BOUND / GRAD_BOUND as they stand, relative to each tensor's max
    |reference|; the measured worst values are printed (DESIGN.md section 43 records them);
  * the batch reduction: the six gradients are the fp32 sum, in image order, of the B single-image launches' gradients,
    byte for byte, for B - 1 = 0, 1, 7, 8, 9, 16 additions and both entry points; an image's tensors do not depend on the batch;
  * sq_partials: each entry against the float64 sum of squares of its slice of the returned gradients at
    (256 + 1) * 2^-24 relative -- 256 roundings of squares and at most 255 of additions of non-negative terms in any order;
  * d_images = NULL and the forward without saved tensors move no bit of what remains."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abi_check as abi
import cnn_edge_cases as E
import test_gpu_cnn as T

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT, SENT8 = 7.0, 0xA5
TAIL = 64
SQ_BOUND = (E.SQ_GROUP + 1) * 2.0 ** -24
ids = lambda c: "B%d-S%d-F%d" % c  # noqa: E731
GRADS = ["d_k1", "d_b1", "d_k2", "d_b2", "d_k3", "d_b3"]                  # in E.NAMES' order
BACKWARD_CASES = [("exact", c) for c in E.EXACT_CASES] + [("real", c) for c in E.INSTANTIATION_REAL]
kids = lambda kc: "%s-%s" % (kc[0], ids(kc[1]))  # noqa: E731


class Guarded:
    """n elements that start as NaN (0xFF) between two rows of sentinels"""

    def __init__(self, n, row, dtype=torch.float32):
        self.n, self.row, self.byte = n, row, dtype == torch.uint8
        self.t = torch.full((n + 2 * row,), SENT8 if self.byte else SENT, dtype=dtype, device="cuda")
        self.t[row:row + n] = 0xFF if self.byte else float("nan")

    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + self.row * self.t.element_size())

    def fetch(self):
        self.whole = self.t.cpu().numpy()
        self.t = None
        return self

    @property
    def inside(self):
        return self.whole[self.row:self.row + self.n]

    def intact(self):
        sent = np.uint8(SENT8) if self.byte else f32(SENT)
        return bool((self.whole[:self.row] == sent).all() and (self.whole[self.row + self.n:] == sent).all())

    def written(self):
        return bool((self.inside != 0xFF).all()) if self.byte else not bool(np.isnan(self.inside).any())


def _input(a, tails):
    """a device copy of `a`; tails: followed by TAIL elements of NaN (0xFF for bytes)"""
    a = np.ascontiguousarray(a).reshape(-1)
    if tails:
        a = np.concatenate([a, np.full(TAIL, 0xFF, np.uint8) if a.dtype == np.uint8 else np.full(TAIL, np.nan, a.dtype)])
    return torch.tensor(a, device="cuda")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _forward(P, images, S, F, save=True, tails=False):
    """air_cnn_fwd -> {out, pool1, pool2, arg1, arg2: Guarded} (the last four absent without `save`)"""
    H = abi.gpu_hip()
    B, n1, n2 = images.shape[0], (S // 2) ** 2 * F, (S // 4) ** 2 * F
    ins = [_input(a, tails) for a in [images] + [P[n] for n in E.NAMES]]
    outs = dict(out=Guarded(B * n2, n2))
    if save:
        outs.update(pool1=Guarded(B * n1, n1), pool2=Guarded(B * n2, n2),
                    arg1=Guarded(B * n1, n1, torch.uint8), arg2=Guarded(B * n2, n2, torch.uint8))
    a = H.CnnFwd(*[_p(t) for t in ins], *[outs[n].ptr() if n in outs else None for n in ("out", "pool1", "pool2", "arg1", "arg2")],
                 B, S, F)
    H.check(H.lib().air_cnn_fwd(C.byref(a), _stream()), "air_cnn_fwd")
    torch.cuda.synchronize()
    return {n: g.fetch() for n, g in outs.items()}


def _backward(entry, P, images, d_out, fwd, S, F, tails=False, d_images=True):
    """air_cnn_bwd / air_cnn_bwd_sq on the forward's own tensors -> {d_images, d_k1 .. d_b3, workspace, sq: Guarded}"""
    H = abi.gpu_hip()
    B, np_ = images.shape[0], E.num_partials(F)
    assert H.lib().air_cnn_workspace_floats(B, S, F) == B * np_
    ins = [_input(a, tails) for a in [d_out.astype(f32), fwd["out"].inside, images, fwd["pool1"].inside, fwd["pool2"].inside,
                                      fwd["arg1"].inside, fwd["arg2"].inside] + [P["cnn/conv%d/kernel" % i] for i in (1, 2, 3)]]
    outs = dict(workspace=Guarded(B * np_, np_), d_k1=Guarded(25 * F, 5 * F), d_b1=Guarded(F, F), d_k2=Guarded(25 * F * F, 5 * F * F),
                d_b2=Guarded(F, F), d_k3=Guarded(25 * F * F, 5 * F * F), d_b3=Guarded(F, F))
    if d_images:
        outs["d_images"] = Guarded(B * S * S, S * S)
    a = H.CnnBwd(*[_p(t) for t in ins], *[outs[n].ptr() for n in ["workspace"] + GRADS],
                 outs["d_images"].ptr() if d_images else None, B, S, F)
    if entry == "air_cnn_bwd_sq":
        nsq = H.lib().air_cnn_num_sq_partials(F)
        outs["sq"] = Guarded(nsq, nsq)
        rc = H.lib().air_cnn_bwd_sq(C.byref(a), outs["sq"].ptr(), _stream())
    else:
        rc = H.lib().air_cnn_bwd(C.byref(a), _stream())
    H.check(rc, entry)
    torch.cuda.synchronize()
    return {n: g.fetch() for n, g in outs.items()}


def _inputs(kind, case):
    return E.exact_case(*case) if kind == "exact" else E.real_case(*case)


@functools.lru_cache(maxsize=None)
def _run(kind, case):
    B, S, F = case
    P, images, d_out, ref = _inputs(kind, case)
    fwd = _forward(P, images, S, F)
    return dict(fwd=fwd, fwd_tails=_forward(P, images, S, F, tails=True),
                bwd=_backward("air_cnn_bwd", P, images, d_out, fwd, S, F),
                bwd_tails=_backward("air_cnn_bwd", P, images, d_out, fwd, S, F, tails=True),
                sq=_backward("air_cnn_bwd_sq", P, images, d_out, fwd, S, F))


@functools.lru_cache(maxsize=None)
def _run_forward(case):
    B, S, F = case
    P, images, ref = E.real_forward_case(*case)
    return dict(fwd=_forward(P, images, S, F), fwd_tails=_forward(P, images, S, F, tails=True))


def _bits(ref):
    return np.ascontiguousarray(ref, np.float64).astype(f32).reshape(-1).tobytes()


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - np.asarray(ref).reshape(-1)).max() / max(np.abs(ref).max(), 1e-300))


# ------------------------------------------------------------------------------------------------- exact-integer cases
@pytest.mark.parametrize("case", E.EXACT_CASES, ids=ids)
def test_exact_forward_has_the_reference_bits(case):
    ref = E.exact_case(*case)[3]
    fwd = _run("exact", case)["fwd"]
    for n in ("arg1", "arg2"):
        assert np.array_equal(fwd[n].inside, ref[n].reshape(-1)), n
    for n in ("pool1", "pool2", "out"):
        assert fwd[n].inside.tobytes() == _bits(ref[n]), n


@pytest.mark.parametrize("entry", ["bwd", "sq"])
@pytest.mark.parametrize("case", E.EXACT_CASES, ids=ids)
def test_exact_backward_has_the_reference_bits(case, entry):
    ref = E.exact_case(*case)[3]
    got = _run("exact", case)[entry]
    assert got["workspace"].inside.tobytes() == _bits(ref["partials"])           # image b's dk1 | db1 | dk2 | db2 | dk3 | db3
    for g, n in zip(GRADS, E.NAMES):
        assert got[g].inside.tobytes() == _bits(ref[n]), n
    assert got["d_images"].inside.tobytes() == _bits(ref["d_images"])


# -------------------------------------------------------------------------------------------------------- every launch
@pytest.mark.parametrize("kc", BACKWARD_CASES, ids=kids)
def test_nothing_lands_outside_and_everything_is_written(kc):
    for launch, outs in _run(*kc).items():
        for n, g in outs.items():
            assert g.intact(), (launch, n)
            assert g.written(), (launch, n)
    B, S, F = kc[1]
    r = _run(*kc)
    assert r["bwd"]["workspace"].n == B * (25 * F + 50 * F * F + 3 * F) and r["sq"]["sq"].n == -(-(25 * F + 50 * F * F + 3 * F) // 256)


@pytest.mark.parametrize("kc", BACKWARD_CASES, ids=kids)
def test_input_tails_move_no_bit(kc):
    r = _run(*kc)
    for plain, tails in (("fwd", "fwd_tails"), ("bwd", "bwd_tails")):
        for n in r[plain]:
            assert r[plain][n].inside.tobytes() == r[tails][n].inside.tobytes(), (plain, n)


@pytest.mark.parametrize("kc", BACKWARD_CASES, ids=kids)
def test_bwd_sq_gradients_and_square_sums(kc):
    """the gradients (and the partials, and d_images) have air_cnn_bwd's bits; sq_partials[i] is the sum of squares of
    slice i of the gradients the launch returned"""
    r = _run(*kc)
    for n in ["workspace", "d_images"] + GRADS:
        assert r["sq"][n].inside.tobytes() == r["bwd"][n].inside.tobytes(), n
    want = E.sq_slices([r["sq"][g].inside for g in GRADS])
    got = r["sq"]["sq"].inside.astype(np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.where(want > 0, want, 1.0)
    print("cnn sq_partials %s: %d entries, last slice %d elements, worst relative error %.3g (bound %.3g)"
          % (kids(kc), got.size, E.num_partials(kc[1][2]) - 256 * (got.size - 1), err.max(), SQ_BOUND))
    assert (got[want == 0] == 0).all() and err.max() <= SQ_BOUND, err
    assert want.max() > 0


# ---------------------------------------------------------------------------------------------------- real-valued cases
@pytest.mark.parametrize("case", E.INSTANTIATION_REAL, ids=ids)
def test_real_forward_and_gradients_against_float64(case):
    ref = E.real_case(*case)[3]
    r = _run("real", case)
    for n in ("arg1", "arg2"):
        assert np.array_equal(r["fwd"][n].inside, ref[n].reshape(-1)), n        # the precondition: the same routing
    fwd = {n: _rel(r["fwd"][n].inside, ref[n]) for n in ("out", "pool1", "pool2")}
    grad = {n: _rel(r["bwd"][g].inside, ref[n]) for g, n in zip(GRADS, E.NAMES)}
    grad["d_images"] = _rel(r["bwd"]["d_images"].inside, ref["d_images"])
    print("cnn edges real %s: forward %.3g (%s), gradients %.3g (%s)"
          % (ids(case), max(fwd.values()), max(fwd, key=fwd.get), max(grad.values()), max(grad, key=grad.get)))
    assert max(fwd.values()) <= T.FWD_BOUND, fwd
    assert max(grad.values()) <= T.GRAD_BOUND, grad


@pytest.mark.parametrize("case", E.REAL_FORWARD_CASES, ids=ids)
def test_real_forward_at_the_limits_against_float64(case):
    ref = E.real_forward_case(*case)[2]
    r = _run_forward(case)
    for launch, outs in r.items():
        for n, g in outs.items():
            assert g.intact() and g.written(), (launch, n)
    for n in r["fwd"]:
        assert r["fwd"][n].inside.tobytes() == r["fwd_tails"][n].inside.tobytes(), n
    errs = {n: _rel(r["fwd"][n].inside, ref[n]) for n in ("out", "pool1", "pool2")}
    print("cnn edges real forward %s: %s" % (ids(case), {k: "%.3g" % v for k, v in errs.items()}))
    assert max(errs.values()) <= T.FWD_BOUND, errs


# -------------------------------------------------------------------------------------------------- the batch reduction
@functools.lru_cache(maxsize=None)
def _single(entry, b):
    """image b of the batch cases alone: (forward, backward through `entry`)"""
    P, images, d_out, ref = E.batch_case(E.BATCH_MAX)
    fwd = _forward(P, images[b:b + 1], E.BATCH_S, E.BATCH_F)
    return fwd, _backward(entry, P, images[b:b + 1], d_out[b:b + 1], fwd, E.BATCH_S, E.BATCH_F)


@functools.lru_cache(maxsize=None)
def _batch(entry, B):
    P, images, d_out, ref = E.batch_case(B)
    fwd = _forward(P, images, E.BATCH_S, E.BATCH_F)
    return fwd, _backward(entry, P, images, d_out, fwd, E.BATCH_S, E.BATCH_F)


@pytest.mark.parametrize("entry", ["air_cnn_bwd", "air_cnn_bwd_sq"])
@pytest.mark.parametrize("B", E.BATCH_SIZES)
def test_batch_reduction_is_the_sequential_fp32_sum(B, entry):
    ref = E.batch_case(B)[3]
    fwd, bwd = _batch(entry, B)
    singles = [_single(entry, b) for b in range(B)]
    for outs in (fwd, bwd):
        for n, g in outs.items():
            assert g.intact() and g.written(), n
    for g, n in zip(GRADS, E.NAMES):
        s = singles[0][1][g].inside.copy()
        for b in range(1, B):
            s = s + singles[b][1][g].inside                                     # fp32, image 0, then + image 1, ...
        assert s.dtype == f32 and bwd[g].inside.tobytes() == s.tobytes(), n
        assert _rel(bwd[g].inside, ref[n]) <= T.GRAD_BOUND, n
    assert _rel(bwd["d_images"].inside, ref["d_images"]) <= T.GRAD_BOUND
    # image b in the batch is image b alone: forward, saved tensors, data gradient, and its partials
    for n in ("out", "pool1", "pool2", "arg1", "arg2"):
        assert fwd[n].inside.tobytes() == b"".join(singles[b][0][n].inside.tobytes() for b in range(B)), n
    for n in ("d_images", "workspace"):
        assert bwd[n].inside.tobytes() == b"".join(singles[b][1][n].inside.tobytes() for b in range(B)), n
    if entry == "air_cnn_bwd_sq":
        other = _batch("air_cnn_bwd", B)[1]
        for g in GRADS:
            assert bwd[g].inside.tobytes() == other[g].inside.tobytes(), g
        want = E.sq_slices([bwd[g].inside for g in GRADS])
        assert (np.abs(bwd["sq"].inside - want) <= SQ_BOUND * want).all()


# -------------------------------------------------------------------------------------------------- optional arguments
@pytest.mark.parametrize("case", E.OPTIONAL_CASES, ids=ids)
def test_optional_arguments_move_no_bit(case):
    B, S, F = case
    P, images, d_out, ref = E.exact_case(*case)
    r = _run("exact", case)
    bare = _forward(P, images, S, F, save=False)
    assert list(bare) == ["out"] and bare["out"].intact() and bare["out"].inside.tobytes() == r["fwd"]["out"].inside.tobytes()
    for entry in ("air_cnn_bwd", "air_cnn_bwd_sq"):
        no_di = _backward(entry, P, images, d_out, r["fwd"], S, F, d_images=False)
        with_di = r["bwd" if entry == "air_cnn_bwd" else "sq"]
        assert "d_images" not in no_di
        for n, g in no_di.items():
            assert g.intact() and g.written(), n
            assert g.inside.tobytes() == with_di[n].inside.tobytes(), (entry, n)
