"""CPU-side checks of the scene source (include/air_hip.h: air_scene_source_*, multi_mnist.DeviceSceneSource): every refusal
is answered on the host before any launch (null device pointers throughout), the Python class refuses what only the host
generator has, and the
device's overlap rule -- as tests/scene_source_cases.py restates it -- accepts exactly the placements the generator's
pixels_overlap / add_buffer accept.  (What the kernel computes: tests/test_gpu_scene_source.py.)"""
import ctypes as C

import numpy as np
import pytest

import abi_check as abi
import scene_source_cases as sc


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def test_limits_are_the_documented_ones(H):
    """(that they are the header's, and the descriptor's layout: tests/test_abi.py, with every other)"""
    assert [H.SCENE_MAX_CANVAS, H.SCENE_MAX_GLYPH, H.SCENE_MAX_DIGITS, H.SCENE_MAX_GAP, H.SCENE_MAX_ATTEMPTS,
            H.SCENE_MAX_RESTARTS] == [128, 32, 6, 4, 100, 64]


def _desc(H, **override):
    """a descriptor that passes every size check, with NULL device pointers"""
    a = H.SceneSource()
    a.B, a.G, a.gd, a.C, a.margin, a.gap, a.max_digits, a.max_attempts, a.max_restarts = 64, 10, 28, 50, 0, 0, 2, 100, 32
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_every_refusal_comes_before_a_launch(H):
    lib = H.lib()
    for fn in (lambda a: lib.air_scene_source_compose(C.byref(a), 0, None), lambda a: lib.air_scene_source_prepare(C.byref(a))):
        assert fn(_desc(H, C=129)) == H.ELIMIT
        assert fn(_desc(H, gd=33)) == H.ELIMIT
        assert fn(_desc(H, max_digits=7)) == H.ELIMIT
        assert fn(_desc(H, gap=5)) == H.ELIMIT
        assert fn(_desc(H, max_attempts=0)) == H.EINVAL
        assert fn(_desc(H, max_attempts=101)) == H.ELIMIT
        assert fn(_desc(H, max_restarts=0)) == H.EINVAL
        assert fn(_desc(H, max_restarts=65)) == H.ELIMIT
        assert fn(_desc(H, B=0)) == H.EINVAL
        assert fn(_desc(H, B=-4)) == H.EINVAL
        assert fn(_desc(H, margin=25)) == H.EINVAL                    # 2 * 25 + 1 > 50: not even one pixel fits
        assert fn(_desc(H, C=16, margin=8)) == H.EINVAL
        for k in ("G", "gd", "C", "max_digits"):
            assert fn(_desc(H, **{k: 0})) == H.EINVAL, k
        assert fn(_desc(H, margin=-1)) == H.EINVAL and fn(_desc(H, gap=-1)) == H.EINVAL
        assert fn(_desc(H, B=0, C=129)) == H.EINVAL                   # an invalid size is reported before a limit
        # the limits themselves pass the size checks: what is left to refuse is the null pointers
        assert fn(_desc(H, C=128, gd=32, max_digits=6, gap=4, max_attempts=100, max_restarts=64, margin=63)) == H.EINVAL
    assert lib.air_scene_source_compose(None, 0, None) == H.EINVAL and lib.air_scene_source_prepare(None) == H.EINVAL
    assert lib.air_scene_source_compose(C.byref(_desc(H)), -1, None) == H.EINVAL
    assert lib.air_scene_source_advance(None, 1, None) == H.EINVAL
    buf = (C.c_int64 * 1)()
    assert lib.air_scene_source_advance(C.addressof(buf), -1, None) == H.EINVAL


def test_each_required_pointer_is_required(H):
    """with every size in range, each null required pointer alone is AIR_EINVAL (bg, counts and gave_up are optional); the
    call with all of them set is not made here -- it would launch"""
    lib = H.lib()
    p = abi.host_ptr().value
    required = ("glyphs", "crops", "batch_counter", "images", "digits", "indices", "positions", "boxes", "status")
    for missing in required:
        a = _desc(H, **{k: p for k in required if k != missing})
        assert lib.air_scene_source_compose(C.byref(a), 0, None) == H.EINVAL, missing
    a = _desc(H, **{k: p for k in required})
    a.crops = p + 4
    assert lib.air_scene_source_compose(C.byref(a), 0, None) == H.EALIGN      # a crop box is one 16-byte load


def test_lds_query(H):
    lds = H.lib().air_scene_source_lds
    up16 = lambda v: (v + 15) // 16 * 16
    for Cv, gd in ((50, 28), (16, 8), (15, 7), (128, 32), (1, 1)):
        assert lds(Cv, gd) == up16(4 * Cv * Cv) + up16(4 * gd * gd) + up16(Cv * Cv) + 160, (Cv, gd)
    assert lds(128, 32) == 86176
    assert lds(129, 8) == H.ELIMIT and lds(50, 33) == H.ELIMIT and lds(0, 8) == H.EINVAL and lds(50, 0) == H.EINVAL


def test_python_class_refuses_jitter_and_box_overlap(H):
    import multi_mnist as mm
    glyphs = sc.ragged_glyphs().reshape(12, 64)
    for kw in (dict(min_w=0.8), dict(max_h=1.2), dict(min_ang=-10.0), dict(max_ang=15.0)):
        with pytest.raises(NotImplementedError, match="Generator.multi_image"):
            mm.DeviceSceneSource(glyphs, 4, None, None, **kw)
    with pytest.raises(NotImplementedError, match="Generator.multi_image"):
        mm.DeviceSceneSource(glyphs, 4, None, None, use_pixel_overlap=False)
    with pytest.raises(TypeError):
        mm.DeviceSceneSource(glyphs, 4, None, None, shear=0.1)
    import torch
    with pytest.raises(H.AirHipError):                                   # no CPU fallback
        mm.DeviceSceneSource(glyphs, 4, torch.zeros(4, 256), torch.zeros(4, dtype=torch.int32), canvas_dim=16)
    assert np.array_equal(mm.crop_boxes(glyphs, 8), sc.crop_boxes(glyphs.reshape(12, 8, 8)))
    with pytest.raises(ValueError, match="empty"):
        mm.crop_boxes(np.zeros((1, 64), np.float32), 8)


@pytest.mark.parametrize("gap", [0, 1, 3])
def test_device_rule_is_the_generators_predicate(gap):
    """200 hand-placed pairs per gap: glyph A on an empty canvas, glyph B offered at (x, y) around it.  The reference
    rejects when max(image, window) != image + window somewhere on the add_buffer-dilated canvas
    (Generator.multi_image: pixels_overlap / add_buffer); the device rejects when an ink pixel of B lies within Chebyshev
    distance `gap` of an ink pixel of A."""
    import multi_mnist as mm
    glyphs = sc.ragged_glyphs()
    crops = sc.crop_boxes(glyphs)
    rng = np.random.RandomState(100 + gap)
    Cn, accepted = 24, 0
    for _ in range(200):
        ga, gb = rng.randint(len(glyphs)), rng.randint(len(glyphs))
        A = glyphs[ga][crops[ga][1]:crops[ga][1] + crops[ga][3], crops[ga][0]:crops[ga][0] + crops[ga][2]]
        Bg = glyphs[gb][crops[gb][1]:crops[gb][1] + crops[gb][3], crops[gb][0]:crops[gb][0] + crops[gb][2]]
        (ha, wa), (hb, wb) = A.shape, Bg.shape
        xa, ya = rng.randint(4, Cn - wa - 3), rng.randint(4, Cn - ha - 3)
        # B's corner within a few pixels of A's box on every side, inside the canvas: overlaps, near misses and clear misses
        x = int(np.clip(xa + rng.randint(-wb - gap - 2, wa + gap + 3), 0, Cn - wb))
        y = int(np.clip(ya + rng.randint(-hb - gap - 2, ha + gap + 3), 0, Cn - hb))
        canvas = np.zeros((Cn, Cn), np.float32)
        canvas[ya:ya + ha, xa:xa + wa] += A
        with_buffer = mm.add_buffer(canvas, gap) if gap > 0 else canvas
        ref_accepts = not mm.pixels_overlap(with_buffer, Bg, x, y)
        dev_accepts = not sc.touches(sc.dilate(canvas > 0, gap), Bg, x, y)
        assert dev_accepts == ref_accepts, (ga, gb, xa, ya, x, y)
        # the rule in words: the smallest Chebyshev distance between an ink pixel of B and one of A exceeds the gap
        pa, pb = np.argwhere(canvas > 0), np.argwhere(Bg > 0) + (y, x)
        dist = np.abs(pa[:, None, :] - pb[None, :, :]).max(-1).min()
        assert dev_accepts == (dist > gap)
        accepted += dev_accepts
    assert 30 < accepted < 170, accepted                                  # both answers are exercised


def test_restatement_draws_and_bounds():
    """the draw stream: word j & 3 of quad j >> 2; range() stays in range; a scene ends within its draw bound"""
    from oracle.philox_ref import philox4x32_10
    d = sc.Draws(b=5, batch=(1 << 32) + 7, seed=(3 << 32) + 9)
    got = [d.next() for _ in range(10)]
    for j, v in enumerate(got):
        assert v == int(philox4x32_10(5, j >> 2, 7, sc.SALT, 9, 3)[j & 3])
    assert all(4 <= sc.Draws(1, 2, 3).range(4, 9) < 13 for _ in range(3))
    glyphs = sc.ragged_glyphs()
    crops = sc.crop_boxes(glyphs)
    assert crops[:, 2:].min() >= 4 and crops[:, 2:].max() <= 7
    out = sc.compose_batch(32, 0, glyphs, crops, 16, 0, 0, 4, 2, 3, seed=1, counts=np.full(32, 4))
    assert (out["status"] == -1).any() and (out["status"] >= 0).any()
    gone = out["status"] == -1
    assert not out["images"][gone].any() and not out["digits"][gone].any() and not out["indices"][gone].any()
    assert (out["digits"][~gone] == 4).all()
