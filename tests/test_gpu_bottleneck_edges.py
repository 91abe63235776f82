"""The two fused VAE-bottleneck launches (air_vae_bottleneck_fwd / _bwd, csrc/air_bottleneck.hip) at their edges: the
bf16 twin outputs, guard space around every output, padded X rows, the twin fall-backs and input rows past M.  The formulas
themselves are checked in test_gpu_kernels.py (test_vae_bottleneck_*); here every check is bits against another launch.

Shapes: M in {5, 16, 37} (less than one 16-row tile, exactly one, two and a ragged third), Z in {2, 50, 64} (one Wml quad;
the model's; every unit lane live -- the exact-fp32 forward stops at 2 Z = 104, so it takes 52 for 64), H of the forward and
K1 of the backward in {8, 200, 256} (one slice with 14 of 16 column quads masked; three full slices and a ragged fourth;
four full ones).  SHAPES is a Latin square over the three: every pair of values meets once."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abi_check as abi

pytestmark = pytest.mark.gpu

K = 256                      # K1 of the forward, H of the backward: the kernels' compile-time width
SHAPES = [(5, 2, 8), (5, 50, 200), (5, 64, 256), (16, 2, 200), (16, 50, 256), (16, 64, 8), (37, 2, 256), (37, 50, 8),
          (37, 64, 200)]
F32_SENTINEL, B16_SENTINEL, B16_NAN = 7.0, 0x1234, 0x7FC0


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _twin(t):
    """RNE bf16 twin as int16 storage (what air_bf16_twin makes: test_bf16_twin_converter_is_rne)"""
    return t.to(torch.bfloat16).view(torch.int16)


def _zmax(form, Z):
    return min(Z, 52) if form == "exact" else Z


@functools.lru_cache(maxsize=None)
def _fwd_operands(M, Z, Hd):
    rng = np.random.RandomState(1000 * M + 10 * Z + Hd)
    t = {k: torch.tensor(v.astype(np.float32), device="cuda") for k, v in dict(
        X=rng.uniform(0, 2, (M, K)), Wml=rng.uniform(-0.1, 0.1, (K, 2 * Z)), bml=rng.uniform(-0.1, 0.1, 2 * Z),
        eps=rng.randn(M, Z), Wg=rng.uniform(-0.3, 0.3, (Z, Hd)), bg=rng.uniform(-0.1, 0.1, Hd)).items()}
    t.update({k + "16": _twin(t[k]) for k in ("X", "Wml", "Wg")})
    return t


@functools.lru_cache(maxsize=None)
def _bwd_operands(H, M, Z, K1):
    rng = np.random.RandomState(2000 * M + 10 * Z + K1)
    att = np.zeros((M, H.ATT_STRIDE))
    att[:, H.ATT_MASK] = rng.randint(0, 2, M)
    dyn = np.zeros(32)
    dyn[H.DYN_GRAD_SCALE], dyn[H.DYN_VAE_PV], dyn[H.DYN_VAE_PM] = 1.0 / 64, 0.8, 0.1
    t = {k: torch.tensor(v.astype(np.float32), device="cuda") for k, v in dict(
        dG=rng.randn(M, K) * 0.1, Wg=rng.uniform(-0.3, 0.3, (Z, K)), ml=rng.uniform(-1, 1, (M, 2 * Z)), eps=rng.randn(M, Z),
        att=att, dyn=dyn, Wml=rng.uniform(-0.1, 0.1, (K1, 2 * Z)), x=rng.uniform(0.01, 2, (M, K1))).items()}
    t.update({k + "16": _twin(t[k]) for k in ("dG", "Wg", "Wml")})
    return t


def _outputs(M, widths, guard, twins):
    """fp32 outputs of the given widths and the bf16 twins of those named in `twins`, sentinel-filled: exactly M rows of
    `width`, or with guard space M + 16 rows of width + 8"""
    rows, pad = (M + 16, 8) if guard else (M, 0)
    o = {k: torch.full((rows * (w + pad),), F32_SENTINEL, device="cuda") for k, w in widths.items()}
    o.update({k + "16": torch.full((rows * (widths[k] + pad),), B16_SENTINEL, dtype=torch.int16, device="cuda") for k in twins})
    return o


def _fwd(H, t, M, Z, Hd, form, twins_out=False, guard=False, ldx=K):
    """one forward launch.  form: "ops" (fp32 operands), "twins" (X16 / Wml16 / Wg16 supplied), "exact" (exact_fp32).
    guard: z / z16 are launched on the [:M, :Z] view of rows of Z + 8; ml and g have no stride and get rows only"""
    o = _outputs(M, dict(ml=2 * Z, z=Z, g=Hd), guard, ("z", "g") if twins_out else ())
    tw = [_p(t[k]) if form == "twins" else None for k in ("X16", "Wml16", "Wg16")]
    a = H.BottleneckFwd(_p(t["X"]), _p(t["Wml"]), _p(t["bml"]), _p(t["eps"]), _p(t["Wg"]), _p(t["bg"]), _p(o["ml"]), _p(o["z"]),
                        _p(o["g"]), M, K, Z, Hd, ldx, _p(o.get("z16")), _p(o.get("g16")), tw[0], tw[1], tw[2], int(form == "exact"),
                        Z + 8 if guard else 0)
    assert H.lib().air_vae_bottleneck_fwd(C.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    return o


def _bwd(H, t, M, Z, K1, form, twins_out=False, guard=False):
    """one backward launch; forms as in _fwd (twins: dG16 / Wg16 / Wml16).  d_ml and d_x have no stride: rows only"""
    o = _outputs(M, dict(d_ml=2 * Z, d_x=K1), guard, ("d_ml", "d_x") if twins_out else ())
    tw = [_p(t[k]) if form == "twins" else None for k in ("dG16", "Wg16", "Wml16")]
    a = H.BottleneckBwd(_p(t["dG"]), _p(t["Wg"]), _p(t["ml"]), _p(t["eps"]), _p(t["att"]), _p(t["dyn"]), _p(t["Wml"]), _p(t["x"]),
                        _p(o["d_ml"]), _p(o["d_x"]), M, K1, Z, K, _p(o.get("d_ml16")), _p(o.get("d_x16")), tw[0], tw[1], tw[2],
                        int(form == "exact"))
    assert H.lib().air_vae_bottleneck_bwd(C.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    return o


def _same(a, b, keys):
    for k in keys:
        assert torch.isfinite(a[k]).all() and torch.equal(a[k], b[k]), k


def _check_twin_outputs(plain, both, keys):
    """the fp32 outputs do not move by a bit when the twin pointers are passed, and each twin is the RNE rounding of
    its sibling"""
    _same(plain, both, keys)
    for k in keys:
        if k + "16" in both:
            assert torch.equal(both[k + "16"].view(torch.bfloat16), both[k].to(torch.bfloat16)), k


def _check_guard(plain, guarded, M, widths, strided, twins_written):
    """every sentinel outside the written region is intact, every value inside is finite and equals the unguarded launch"""
    for k, w in widths.items():
        for name, sentinel in ((k, F32_SENTINEL), (k + "16", B16_SENTINEL)):
            if name not in guarded:
                continue
            buf = guarded[name]
            inside = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
            if k in strided:
                inside.view(M + 16, w + 8)[:M, :w] = True
            else:
                inside[:M * w] = True
            if name.endswith("16") and not twins_written:      # exact forms: twins ignored, not written
                inside[:] = False
            assert bool((buf[~inside] == sentinel).all()), name
            if inside.any():
                assert name.endswith("16") or torch.isfinite(buf[inside]).all(), name
                assert torch.equal(buf[inside], plain[name]), name


@pytest.mark.parametrize("form", ["ops", "twins"])
@pytest.mark.parametrize("M,Z,Hd", SHAPES)
def test_forward_twin_outputs_are_the_rne_rounding_of_their_siblings(H, M, Z, Hd, form):
    t = _fwd_operands(M, Z, Hd)
    _check_twin_outputs(_fwd(H, t, M, Z, Hd, form), _fwd(H, t, M, Z, Hd, form, twins_out=True), ("ml", "z", "g"))


@pytest.mark.parametrize("form", ["ops", "twins"])
@pytest.mark.parametrize("M,Z,K1", SHAPES)
def test_backward_twin_outputs_are_the_rne_rounding_of_their_siblings(H, M, Z, K1, form):
    t = _bwd_operands(H, M, Z, K1)
    _check_twin_outputs(_bwd(H, t, M, Z, K1, form), _bwd(H, t, M, Z, K1, form, twins_out=True), ("d_ml", "d_x"))


@pytest.mark.parametrize("form", ["ops", "twins", "exact"])
@pytest.mark.parametrize("M,Z,Hd", SHAPES)
def test_forward_outputs_stay_inside_their_rows_and_columns(H, M, Z, Hd, form):
    Z = _zmax(form, Z)
    t = _fwd_operands(M, Z, Hd)
    plain = _fwd(H, t, M, Z, Hd, form, twins_out=True)
    _check_guard(plain, _fwd(H, t, M, Z, Hd, form, twins_out=True, guard=True), M, dict(ml=2 * Z, z=Z, g=Hd), ("z",),
                 form != "exact")


@pytest.mark.parametrize("form", ["ops", "twins", "exact"])
@pytest.mark.parametrize("M,Z,K1", SHAPES)
def test_backward_outputs_stay_inside_their_rows(H, M, Z, K1, form):
    t = _bwd_operands(H, M, Z, K1)
    plain = _bwd(H, t, M, Z, K1, form, twins_out=True)
    _check_guard(plain, _bwd(H, t, M, Z, K1, form, twins_out=True, guard=True), M, dict(d_ml=2 * Z, d_x=K1), (), form != "exact")


@pytest.mark.parametrize("ldx", [264, 260])
def test_forward_padded_x_rows_ignore_what_the_pad_holds(H, ldx):
    """X in rows of 264 floats (ldx % 8 == 0: the twin form is eligible) and of 260 (ldx % 4 == 0 only: with twins supplied
    the call falls back to the fp32-operand instance), NaN in the pad columns of X and of X16: the bits of ldx = 256"""
    M, Z, Hd = 37, 50, 200
    t = _fwd_operands(M, Z, Hd)
    tp = dict(t)
    tp["X"] = torch.full((M, ldx), float("nan"), device="cuda")
    tp["X"][:, :K] = t["X"]
    tp["X16"] = torch.full((M, ldx), B16_NAN, dtype=torch.int16, device="cuda")
    tp["X16"][:, :K] = t["X16"]
    for form in ("ops", "twins", "exact"):
        _same(_fwd(H, t, M, Z, Hd, form, twins_out=form != "exact"), _fwd(H, tp, M, Z, Hd, form, twins_out=form != "exact", ldx=ldx),
              ("ml", "z", "g") + (("z16", "g16") if form != "exact" else ()))
    _same(_fwd(H, t, M, Z, Hd, "ops"), _fwd(H, tp, M, Z, Hd, "twins", ldx=ldx), ("ml", "z", "g"))


def _offset_copy(t, off):
    """the same values at an address `off` elements past an aligned one"""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


@pytest.mark.parametrize("M,Z,Hd", [(37, 50, 200), (5, 2, 8)])
def test_forward_twin_fall_back_by_alignment(H, M, Z, Hd):
    """Wml16 at a 2-byte aligned address: the call returns 0 and gives the bits of a call without twins"""
    t = _fwd_operands(M, Z, Hd)
    tp = dict(t, Wml16=_offset_copy(t["Wml16"], 1))
    _same(_fwd(H, t, M, Z, Hd, "ops", twins_out=True), _fwd(H, tp, M, Z, Hd, "twins", twins_out=True), ("ml", "z", "g", "z16", "g16"))


@pytest.mark.parametrize("M,Z,K1", [(37, 50, 200), (5, 2, 8)])
def test_backward_twin_fall_back_by_alignment(H, M, Z, K1):
    """dG16 at an address that is 8-byte aligned and not 16: returns 0, the bits of a call without twins"""
    t = _bwd_operands(H, M, Z, K1)
    tp = dict(t, dG16=_offset_copy(t["dG16"], 4))
    _same(_bwd(H, t, M, Z, K1, "ops", twins_out=True), _bwd(H, tp, M, Z, K1, "twins", twins_out=True),
          ("d_ml", "d_x", "d_ml16", "d_x16"))


def _nan_rows_after(t, keys, M):
    """the M real rows of each operand followed by NaN rows up to 16"""
    out = dict(t)
    for k in keys:
        nan = B16_NAN if t[k].dtype == torch.int16 else float("nan")
        out[k] = torch.full((16,) + tuple(t[k].shape[1:]), nan, dtype=t[k].dtype, device="cuda")
        out[k][:M] = t[k]
    return out


@pytest.mark.parametrize("form", ["ops", "twins", "exact"])
@pytest.mark.parametrize("Z,Hd", [(50, 200), (2, 8), (64, 256)])
def test_forward_never_consumes_input_rows_past_m(H, Z, Hd, form):
    M, Z = 5, _zmax(form, Z)
    t = _fwd_operands(M, Z, Hd)
    tw = form != "exact"
    _same(_fwd(H, t, M, Z, Hd, form, twins_out=tw), _fwd(H, _nan_rows_after(t, ("X", "X16", "eps"), M), M, Z, Hd, form, twins_out=tw),
          ("ml", "z", "g") + (("z16", "g16") if tw else ()))


@pytest.mark.parametrize("form", ["ops", "twins", "exact"])
@pytest.mark.parametrize("Z,K1", [(50, 200), (2, 8), (64, 256)])
def test_backward_never_consumes_input_rows_past_m(H, Z, K1, form):
    M = 5
    t = _bwd_operands(H, M, Z, K1)
    tw = form != "exact"
    _same(_bwd(H, t, M, Z, K1, form, twins_out=tw),
          _bwd(H, _nan_rows_after(t, ("dG", "dG16", "eps", "ml", "att", "x"), M), M, Z, K1, form, twins_out=tw),
          ("d_ml", "d_x") + (("d_ml16", "d_x16") if tw else ()))
