"""CPU-side checks of the segmentation metrics (include/air_hip.h: air_scene_masks, air_segmentation*, air/metrics.py,
training.py --segmentation): exports and binding, the descriptors against a C compile of the header, every refusal on the
host before any launch, in the stated order, with host pointers that are never dereferenced -- no descriptor that would
launch is passed; the workspace query; the Python class's refusals; the driver's refusal where no source composes the test
set.  (What the kernels compute: tests/test_gpu_segmentation.py.)"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import abi_check as abi
import segmentation_cases as sc

SEG_REQUIRED = ("att", "vrec", "gt_mask", "counts", "sums")
SEG_OPTIONAL = ("pred_mask", "tables", "ari", "mask_iou")
MASK_POINTERS = ("glyphs", "crops", "digits", "indices", "positions", "mask")


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _seg(H, ptrs=True, **override):
    """a descriptor that would pass every check (so it is only ever sent with something wrong)"""
    a = H.Segmentation()
    a.T, a.B, a.k, a.G, a.C, a.w, a.pred_threshold = 3, 64, 64, 2, 50, 28, 0.5
    if ptrs:
        for k in SEG_REQUIRED + SEG_OPTIONAL:
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def _masks(H, ptrs=True, **override):
    a = H.SceneMasks()
    a.B, a.G, a.gd, a.C, a.max_digits, a.ink_threshold = 8, 10, 28, 50, 2, 0.0
    if ptrs:
        for k in MASK_POINTERS:
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_exports_binding_and_the_documented_constants(H):
    lib = C.CDLL(H.LIB_PATH)
    for name in ("air_scene_masks", "air_segmentation", "air_segmentation_workspace_bytes"):
        assert hasattr(lib, name) and name in H.EXPORTED_SYMBOLS, name
    assert H.lib().air_abi_version() == 6                       # additive
    assert (H.SEG_MAX_STEPS, H.SEG_MAX_DIGITS, H.SEG_MAX_CANVAS, H.SEG_MAX_WINDOW) == (16, 16, 128, 32) == \
        (sc.MAX_STEPS, sc.MAX_DIGITS, sc.MAX_CANVAS, sc.MAX_WINDOW)
    assert H.LOC_GROUP == sc.GROUP == 256                       # the summation group is air_localization's
    assert (H.SEG_IMAGES, H.SEG_SCORED, H.SEG_PRESENT, H.SEG_FG_PIXELS, H.SEG_FG_MISSED, H.SEG_BG_CLAIMED, H.SEG_COUNTS) == \
        (sc.IMAGES, sc.SCORED, sc.PRESENT, sc.FG_PIXELS, sc.FG_MISSED, sc.BG_CLAIMED, sc.COUNTS)
    assert (H.SEG_ARI, H.SEG_MASK_IOU, H.SEG_SUMS) == (sc.ARI, sc.MASK_IOU, sc.SUMS)
    assert (H.ATT_S, H.ATT_X, H.ATT_Y, H.ATT_Z, H.ATT_MASK, H.ATT_STRIDE) == \
        (sc.ATT_S, sc.ATT_X, sc.ATT_Y, sc.ATT_Z, sc.ATT_MASK, sc.ATT_STRIDE)
    assert (H.SCENE_MAX_CANVAS, H.SCENE_MAX_GLYPH, H.SCENE_MAX_DIGITS) == (128, 32, 6)
    # the scene-mask descriptor names the scene source's arrays as the scene source does
    assert {"glyphs", "crops", "digits", "indices", "positions"} <= {f[0] for f in H.SceneSource._fields_}


def test_structs_match_a_c_compile_of_the_header(H):
    h, num = abi.read_header(), abi.compile_numbers()
    for ctype, cls in (("air_segmentation_t", H.Segmentation), ("air_scene_masks_t", H.SceneMasks)):
        assert h.structs[ctype] == [f[0] for f in cls._fields_] and num.sizeof[ctype] == C.sizeof(cls), ctype
        for name, ftype in cls._fields_:
            assert num.fields[ctype, name] == (getattr(cls, name).offset, C.sizeof(ftype)), (ctype, name)
    assert h.prototypes["air_segmentation"] == ("int", ["const air_segmentation_t*", "void*", "void*"])
    assert h.prototypes["air_scene_masks"] == ("int", ["const air_scene_masks_t*", "void*"])
    assert h.prototypes["air_segmentation_workspace_bytes"] == ("int64_t", ["int"] * 4)
    assert abi.check_abi(H) == []


def test_the_kernels_have_rows_in_the_table_of_kernel_names(H):
    from air import air_model as am
    assert am.KERNEL_NAMES["air_segmentation"] == "seg_image_kernel" and am.KERNEL_NAMES["air_scene_masks"] == "scene_masks_kernel"


def test_segmentation_refuses_before_a_launch_and_in_order(H):
    lib, ws = H.lib(), abi.host_ptr()
    call = lambda a, w=ws: lib.air_segmentation(C.byref(a), w, None)      # noqa: E731
    assert lib.air_segmentation(None, ws, None) == H.EINVAL
    for k in ("T", "B", "k", "G"):
        assert call(_seg(H, **{k: 0})) == H.EINVAL and call(_seg(H, **{k: -2})) == H.EINVAL, k
    assert call(_seg(H, k=65)) == H.EINVAL                                # k > B
    assert call(_seg(H, T=17)) == H.ELIMIT and call(_seg(H, G=17)) == H.ELIMIT
    for k in ("C", "w"):
        assert call(_seg(H, **{k: 1})) == H.EINVAL and call(_seg(H, **{k: 0})) == H.EINVAL and call(_seg(H, **{k: -5})) == H.EINVAL, k
    assert call(_seg(H, C=129)) == H.ELIMIT and call(_seg(H, w=33)) == H.ELIMIT
    for thr in (-0.001, 1.0, 1.5, float("nan"), float("inf"), -float("inf")):
        assert call(_seg(H, pred_threshold=thr)) == H.EINVAL, thr
    for missing in SEG_REQUIRED:
        assert call(_seg(H, **{missing: None})) == H.EINVAL, missing
    assert call(_seg(H), None) == H.EINVAL                                # no workspace
    assert call(_seg(H, ptrs=False)) == H.EINVAL
    # the order: a size before a limit; the step and digit limits before the canvas and the window; their sizes before
    # their limits; every limit before the threshold and the pointers
    assert call(_seg(H, T=17, k=0)) == H.EINVAL and call(_seg(H, G=17, k=65)) == H.EINVAL
    assert call(_seg(H, T=17, C=1)) == H.ELIMIT and call(_seg(H, G=17, w=0)) == H.ELIMIT
    assert call(_seg(H, C=129, w=1)) == H.EINVAL and call(_seg(H, C=1, w=33)) == H.EINVAL
    assert call(_seg(H, ptrs=False, T=17)) == H.ELIMIT and call(_seg(H, ptrs=False, C=129)) == H.ELIMIT
    assert call(_seg(H, w=33, pred_threshold=2.0), None) == H.ELIMIT
    assert call(_seg(H, ptrs=False, pred_threshold=float("nan"))) == H.EINVAL


def test_scene_masks_refuses_before_a_launch_and_in_order(H):
    lib = H.lib()
    call = lambda a: lib.air_scene_masks(C.byref(a), None)                # noqa: E731
    assert lib.air_scene_masks(None, None) == H.EINVAL
    for k in ("B", "G", "gd", "C", "max_digits"):
        assert call(_masks(H, **{k: 0})) == H.EINVAL and call(_masks(H, **{k: -3})) == H.EINVAL, k
    for thr in (-0.5, float("nan"), -float("inf")):
        assert call(_masks(H, ink_threshold=thr)) == H.EINVAL, thr
    assert call(_masks(H, C=129)) == H.ELIMIT and call(_masks(H, gd=33)) == H.ELIMIT and call(_masks(H, max_digits=7)) == H.ELIMIT
    for missing in MASK_POINTERS:
        assert call(_masks(H, **{missing: None})) == H.EINVAL, missing
    # sizes before limits before null pointers
    assert call(_masks(H, C=129, B=0)) == H.EINVAL and call(_masks(H, gd=33, ink_threshold=-1.0)) == H.EINVAL
    assert call(_masks(H, ptrs=False, C=129)) == H.ELIMIT and call(_masks(H, ptrs=False, max_digits=7)) == H.ELIMIT
    assert call(_masks(H, ptrs=False)) == H.EINVAL


def test_workspace_query_answers_as_the_entry_point(H):
    q = H.lib().air_segmentation_workspace_bytes
    for T, B, k, G in ((1, 1, 1, 1), (3, 8, 5, 2), (16, 7, 7, 16), (3, 1000, 1000, 2), (3, 260, 257, 2)):
        assert q(T, B, k, G) == k * sc.WORKSPACE_BYTES_PER_IMAGE, (T, B, k, G)
    assert q(3, 2 ** 31 - 1, 2 ** 31 - 1, 2) == (2 ** 31 - 1) * 56      # no overflow at the largest batch
    for bad in ((0, 8, 8, 2), (3, 0, 0, 2), (3, 8, 0, 2), (3, 8, 8, 0), (3, 8, 9, 2), (-1, 8, 8, 2)):
        assert q(*bad) == H.EINVAL, bad
    assert q(17, 8, 8, 2) == H.ELIMIT and q(3, 8, 8, 17) == H.ELIMIT and q(16, 8, 8, 16) == 448
    assert q(17, 8, 9, 2) == H.EINVAL                                      # a size before a limit


def _stub(max_steps=3, batch_size=8, canvas_size=50, windows_size=28, device_tensor=None):
    return types.SimpleNamespace(max_steps=max_steps, batch_size=batch_size, canvas_size=canvas_size, windows_size=windows_size,
                                 input_images=torch.zeros(batch_size, canvas_size ** 2) if device_tensor is None else device_tensor)


def test_python_class_refuses_on_the_host(H):
    from air.metrics import Segmentation
    assert Segmentation.names() == list(sc.NAMES)
    with pytest.raises(NotImplementedError, match="holds 16 and 16"):
        Segmentation(_stub(max_steps=17), 2)
    with pytest.raises(NotImplementedError, match="holds 16 and 16"):
        Segmentation(_stub(), 17)
    with pytest.raises(NotImplementedError, match="holds 128 and 32"):
        Segmentation(_stub(canvas_size=129), 2)
    with pytest.raises(NotImplementedError, match="holds 128 and 32"):
        Segmentation(_stub(windows_size=33), 2)
    with pytest.raises(ValueError, match="max_gt_digits"):
        Segmentation(_stub(), 0)
    for thr in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="pred_threshold"):
            Segmentation(_stub(), 2, pred_threshold=thr)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):           # valid arguments: what is missing is a device tensor
        Segmentation(_stub(), 2)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        Segmentation(_stub(device_tensor=np.zeros((8, 2500), np.float32)), 2, keep=True)
    s = sc.hand_scene()
    arrays = {k: torch.from_numpy(s[k]) for k in ("glyphs", "crops", "indices", "positions")}
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        Segmentation.scene_masks(dict(arrays, canvas_dim=s["C"]), torch.from_numpy(s["digits"]))


def test_colour_masks_follows_the_box_colours():
    from air.visualize import colour_masks
    mask = torch.tensor([[0, 1, 2, 3, 4, 0, 0, 0, 0]], dtype=torch.uint8)
    canvas = torch.full((1, 9), 0.25)
    rgb = colour_masks(mask, canvas)
    assert tuple(rgb.shape) == (1, 3, 3, 3)
    flat = rgb.reshape(9, 3).tolist()
    assert flat[0] == [0.25] * 3 and flat[1] == [1, 0, 0] and flat[2] == [0, 1, 0] and flat[3] == [0, 0, 1] and flat[4] == [1, 0, 0]
    assert colour_masks(mask.reshape(1, 3, 3), 3).reshape(9, 3).tolist()[0] == [0, 0, 0]


def test_training_refuses_segmentation_without_a_device_test_set(tmp_path):
    """parser.error (exit status 2) before anything touches a device or the results folder"""
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "training.py")
    for extra in ([], ["--online-data"]):
        p = subprocess.run([sys.executable, script, "--segmentation", "-r", str(tmp_path / "out")] + extra, cwd=str(tmp_path),
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 2 and "glyph table of the composing source" in p.stderr, (p.returncode, p.stderr[-400:])
        assert not (tmp_path / "out").exists()
    p = subprocess.run([sys.executable, script, "--segmentation", "--online-data", "--glyph-style", "mnist-like",
                        "--segmentation-threshold", "1"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--segmentation-threshold" in p.stderr
