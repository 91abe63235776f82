"""CPU-side checks of the handwriting bank (include/air_hip.h: air_glyph_distort*, multi_mnist.DeviceHandwritingBank): every
refusal is answered on the host before any launch, in the stated order (an invalid size before a limit, a limit before a null
pointer, a null pointer before the alignment), with host pointers that are never dereferenced; the LDS query; the Python
class's refusals.  (What the kernel computes: tests/test_gpu_glyph_distort.py; the descriptor's layout and the signatures:
tests/test_abi.py, with every other.)"""
import ctypes as C

import numpy as np
import pytest

import abi_check as abi
import glyph_distort_cases as gd
import scene_source_cases as sc

POINTERS = ("glyphs", "taps", "bank", "bank_crops", "source", "params", "status")        # counter is optional


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _desc(H, ptrs=True, **override):
    """a descriptor that passes every check (the preset's shapes and bounds); ptrs: the required pointers set to a host
    address the checks never follow"""
    a = H.GlyphDistort()
    a.V, a.G, a.gd, a.od, a.ink, a.radius, a.min_stroke, a.max_stroke = 4096, 1797, 40, 28, 20, 24, -1, 1
    a.field_gain, a.max_ang, a.max_shear, a.min_scale, a.max_scale, a.lo, a.hi = 25.0, 12.0, 0.2, 0.85, 1.15, 0.3, 0.7
    if ptrs:
        for k in POINTERS:
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_the_limits_are_the_documented_ones(H):
    assert (H.DISTORT_MAX_PLANE, H.DISTORT_MAX_RADIUS, H.DISTORT_MAX_STROKE) == (40, 64, 4) == (gd.MAX_PLANE, gd.MAX_RADIUS, gd.MAX_STROKE)
    assert H.DISTORT_MAX_PLANE >= 40 and H.DISTORT_MAX_RADIUS >= H.DISTORT_MAX_PLANE      # a tap line wider than the plane
    assert H.SCENE_MAX_GLYPH == 32


def test_the_kernel_has_a_row_in_the_table_of_kernel_names(H):
    from air import air_model as am
    assert am.KERNEL_NAMES["air_glyph_distort"] == "glyph_distort_kernel"


def test_a_valid_descriptor_passes_the_checks(H):
    """below 48 KiB of LDS prepare is the checks alone: 0, and nothing was launched (no device here); counter may be null"""
    prepare = H.lib().air_glyph_distort_prepare
    assert prepare(C.byref(_desc(H))) == 0
    assert prepare(C.byref(_desc(H, counter=abi.host_ptr().value))) == 0
    neutral = _desc(H, field_gain=0.0, max_ang=0.0, max_shear=0.0, min_scale=1.0, max_scale=1.0, min_stroke=0, max_stroke=0,
                    lo=0.0, hi=1.0, radius=0)
    assert prepare(C.byref(neutral)) == 0
    # the limits themselves pass
    edge = _desc(H, V=1, G=1, gd=40, od=32, ink=32, radius=64, min_stroke=-4, max_stroke=4, max_ang=180.0)
    assert prepare(C.byref(edge)) == 0
    for kw in (dict(max_ang=-180.0), dict(max_shear=-0.5), dict(gd=1, od=1, ink=1), dict(ink=28), dict(min_scale=1e-300),
               dict(field_gain=-3.0), dict(lo=-1.0, hi=-0.5), dict(min_stroke=3, max_stroke=3)):
        assert prepare(C.byref(_desc(H, **kw))) == 0, kw


def test_every_refusal_comes_before_a_launch(H):
    """(only refused descriptors go to air_glyph_distort itself: one that passes would launch on host pointers)"""
    lib = H.lib()
    inf, nan = float("inf"), float("nan")
    for fn in (lambda a: lib.air_glyph_distort(C.byref(a), None), lambda a: lib.air_glyph_distort_prepare(C.byref(a))):
        for k in ("V", "G", "gd", "od", "ink"):
            assert fn(_desc(H, **{k: 0})) == H.EINVAL and fn(_desc(H, **{k: -3})) == H.EINVAL, k
        assert fn(_desc(H, radius=-1)) == H.EINVAL
        assert fn(_desc(H, ink=29)) == H.EINVAL                                      # ink > od
        for k in ("field_gain", "max_ang", "max_shear", "min_scale", "max_scale", "lo", "hi"):
            assert fn(_desc(H, **{k: nan})) == H.EINVAL and fn(_desc(H, **{k: inf})) == H.EINVAL, k
            assert fn(_desc(H, **{k: -inf})) == H.EINVAL, k
        assert fn(_desc(H, min_scale=1.2, max_scale=1.1)) == H.EINVAL
        assert fn(_desc(H, min_stroke=2, max_stroke=1)) == H.EINVAL
        assert fn(_desc(H, lo=0.7, hi=0.7)) == H.EINVAL and fn(_desc(H, lo=0.8, hi=0.7)) == H.EINVAL
        assert fn(_desc(H, min_scale=0.0)) == H.EINVAL and fn(_desc(H, min_scale=-2.0, max_scale=-1.0)) == H.EINVAL
        # limits
        assert fn(_desc(H, gd=41)) == H.ELIMIT and fn(_desc(H, od=33, ink=20)) == H.ELIMIT
        assert fn(_desc(H, radius=65)) == H.ELIMIT
        assert fn(_desc(H, max_ang=180.5)) == H.ELIMIT and fn(_desc(H, max_ang=-181.0)) == H.ELIMIT
        assert fn(_desc(H, min_stroke=-5)) == H.ELIMIT and fn(_desc(H, max_stroke=5)) == H.ELIMIT
        # the order: an invalid size before a limit, a limit before a null pointer, a null pointer before the alignment
        assert fn(_desc(H, V=0, gd=41)) == H.EINVAL
        assert fn(_desc(H, lo=nan, max_ang=200.0)) == H.EINVAL
        assert fn(_desc(H, min_scale=0.0, radius=65)) == H.EINVAL
        assert fn(_desc(H, od=33, ink=33)) == H.ELIMIT and fn(_desc(H, od=33, ink=34)) == H.EINVAL
        assert fn(_desc(H, ptrs=False, gd=41)) == H.ELIMIT and fn(_desc(H, ptrs=False, max_stroke=5)) == H.ELIMIT
        assert fn(_desc(H, ptrs=False)) == H.EINVAL
        assert fn(_desc(H, glyphs=None, bank_crops=abi.host_ptr().value + 4)) == H.EINVAL
    assert lib.air_glyph_distort(None, None) == H.EINVAL and lib.air_glyph_distort_prepare(None) == H.EINVAL


def test_each_required_pointer_is_required_and_aligned(H):
    """prepare alone from here on: with every pointer set, air_glyph_distort itself would launch"""
    prepare = H.lib().air_glyph_distort_prepare
    for missing in POINTERS:
        assert prepare(C.byref(_desc(H, **{missing: None}))) == H.EINVAL, missing
    p = abi.host_ptr().value
    assert prepare(C.byref(_desc(H, bank_crops=p + 4))) == H.EALIGN and prepare(C.byref(_desc(H, bank_crops=p + 8))) == H.EALIGN
    for k in ("params", "taps"):
        assert prepare(C.byref(_desc(H, **{k: p + 4}))) == H.EALIGN and prepare(C.byref(_desc(H, **{k: p + 8}))) == 0, k
    assert prepare(C.byref(_desc(H, glyphs=p + 4, bank=p + 4, source=p + 4, status=p + 4))) == 0


def test_lds_query(H):
    lds = H.lib().air_glyph_distort_lds
    want = lambda g, o, r: 3 * 8 * max(g, o) ** 2 + 8 * (2 * r + 1) + 4 * max(g, o) ** 2 + 32
    for g, o, r in ((40, 28, 24), (40, 32, 64), (8, 16, 9), (24, 28, 24), (1, 1, 0), (8, 16, 0), (7, 9, 3)):
        assert lds(g, o, r) == want(g, o, r), (g, o, r)
    assert lds(40, 28, 24) == 45224 and lds(40, 32, 64) == 45864 <= 48 * 1024      # the limits need no grant
    assert lds(0, 8, 1) == H.EINVAL and lds(8, 0, 1) == H.EINVAL and lds(8, 8, -1) == H.EINVAL
    assert lds(41, 28, 1) == H.ELIMIT and lds(8, 33, 1) == H.ELIMIT and lds(8, 8, 65) == H.ELIMIT and lds(0, 33, 1) == H.EINVAL


def test_python_bank_refuses_on_the_host(H):
    import multi_mnist as mm
    glyphs = sc.ragged_glyphs().reshape(12, 64)
    for kw, code in ((dict(min_scale=1.2, max_scale=1.1), "-1"), (dict(min_scale=0.0), "-1"), (dict(max_ang=float("nan")), "-1"),
                     (dict(ink=17), "-1"), (dict(lo=0.5, hi=0.5), "-1"), (dict(min_stroke=1, max_stroke=0), "-1"),
                     (dict(od=33, ink=20), "-2"), (dict(max_ang=200.0), "-2"), (dict(max_stroke=5), "-2"),
                     (dict(sigma=20.0), "-2"), (dict(radius=65), "-2"), (dict(variants=0), "-1")):
        args = dict(variants=16, od=16, ink=10)
        args.update(kw)
        with pytest.raises(H.AirHipError, match="air_glyph_distort_prepare failed with code %s" % code):
            mm.DeviceHandwritingBank(glyphs, **args)
    with pytest.raises(H.AirHipError, match="code -2"):
        mm.DeviceHandwritingBank(np.zeros((2, 41 * 41), np.float32), 16)                # gd = 41
    with pytest.raises(ValueError, match=">= 0"):
        mm.DeviceHandwritingBank(-glyphs, 16, od=16, ink=10)
    with pytest.raises(ValueError, match="<= 1"):
        mm.DeviceHandwritingBank(glyphs * 2, 16, od=16, ink=10)
    with pytest.raises(ValueError, match="gd \\* gd"):
        mm.DeviceHandwritingBank(glyphs[:, :63], 16, od=16, ink=10)
    for kw in (dict(sigma=0.0), dict(sigma=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(ValueError, match="sigma"):
            mm.DeviceHandwritingBank(glyphs, 16, od=16, ink=10, **kw)
    with pytest.raises(TypeError):
        mm.DeviceHandwritingBank(glyphs, 16, min_w=0.9)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):                       # valid arguments: what is missing is a GPU
        mm.DeviceHandwritingBank(glyphs, 16, od=16, ink=10, device="cpu", **gd.MNIST_LIKE)


def test_host_side_taps_and_gain_are_the_restatements(H):
    import multi_mnist as mm
    for sigma, radius in ((6.0, None), (2.0, 9), (1.0, 0), (0.7, None)):
        taps, R = mm.gaussian_taps(sigma, radius)
        want, wantR = gd.gaussian_taps(sigma, radius)
        assert R == wantR and np.array_equal(taps, want)
    assert mm.gaussian_taps(6.0)[1] == 24 and mm.gaussian_taps(1.0, 0)[0].tolist() == [1.0]


def test_scene_source_still_refuses_jitter_keywords_and_the_preset_is_the_issues(H):
    import multi_mnist as mm
    glyphs = sc.ragged_glyphs().reshape(12, 64)
    with pytest.raises(NotImplementedError, match="Generator.multi_image"):
        mm.DeviceSceneSource(glyphs, 4, None, None, min_w=0.8)
    assert mm.MNIST_LIKE == dict(side=40, ink=20, od=28, sigma=6.0, alpha=1.5, max_ang=12.0, max_shear=0.2, min_scale=0.85,
                                 max_scale=1.15, min_stroke=-1, max_stroke=1, lo=0.3, hi=0.7)
    with pytest.raises(ValueError, match="glyph_style"):
        mm.compose_on_device(8, glyph_style="cursive")


def test_drivers_refuse_the_style_with_jitter_flags_or_without_the_device(H):
    """parser.error (exit status 2) before anything touches a device"""
    import os
    import subprocess
    import sys
    pkg = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd")
    for cmd, message in (
            (["training.py", "--online-data", "--glyph-style", "mnist-like", "--min-width-scale", "0.9"], "leave the scale / rotation flags neutral"),
            (["training.py", "--online-data", "--glyph-style", "mnist-like", "--max-rotation-angle", "15"], "leave the scale / rotation flags neutral"),
            (["training.py", "--glyph-style", "mnist-like"], "give --online-data"),
            (["training.py", "--online-data", "--glyph-style", "cursive"], "invalid choice"),
            (["multi_mnist.py", "--device", "8", "--glyph-style", "mnist-like", "--max-height-scale", "1.2"], "leave the scale / rotation flags neutral"),
            (["multi_mnist.py", "--glyph-style", "mnist-like"], "give --device N")):
        p = subprocess.run([sys.executable] + cmd, cwd=pkg, capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and message in p.stderr, (cmd, p.returncode, p.stderr[-300:])
