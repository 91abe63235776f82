"""CPU-side checks of the localisation metrics (include/air_hip.h: air_localization*, air/metrics.py, training.py
--localization): every refusal is answered on the host before any launch, in the stated order, with host pointers that are
never dereferenced -- no descriptor that would launch is passed; the workspace query; the Python class's refusals; the
driver's refusal of a cache without ground truth.  (What the kernel computes: tests/test_gpu_localization.py; the
descriptor's layout and the signatures: tests/test_abi.py, with every other.)"""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import abi_check as abi
import localization_cases as lc

REQUIRED = ("att", "run_digits", "gt_count", "gt_positions", "gt_boxes", "counts", "sums")


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def _desc(H, ptrs=True, **override):
    """a descriptor that would pass every check (so it is only ever sent with something wrong)"""
    a = H.Localization()
    a.T, a.B, a.k, a.G, a.canvas_size, a.iou_threshold = 3, 64, 64, 2, 50, 0.5
    if ptrs:
        for k in REQUIRED + ("match", "iou"):
            setattr(a, k, abi.host_ptr().value)
    for k, v in override.items():
        setattr(a, k, v)
    return a


def test_the_limits_and_the_layout_are_the_documented_ones(H):
    assert (H.LOC_MAX_STEPS, H.LOC_MAX_DIGITS, H.LOC_GROUP) == (16, 16, 256) == (lc.MAX_STEPS, lc.MAX_DIGITS, lc.GROUP)
    assert (H.LOC_IMAGES, H.LOC_PRESENT, H.LOC_INFERRED, H.LOC_MATCHED, H.LOC_HITS, H.LOC_COUNT_CORRECT, H.LOC_COUNTS) == \
        (lc.IMAGES, lc.PRESENT, lc.INFERRED, lc.MATCHED, lc.HITS, lc.COUNT_CORRECT, lc.COUNTS)
    assert (H.LOC_IOU, H.LOC_COVER, H.LOC_DIST, H.LOC_SUMS) == (lc.IOU, lc.COVER, lc.DIST, lc.SUMS)
    assert (H.ATT_S, H.ATT_X, H.ATT_Y, H.ATT_STRIDE) == (lc.ATT_S, lc.ATT_X, lc.ATT_Y, lc.ATT_STRIDE)
    assert H.lib().air_abi_version() == 6                       # additive
    # the first five fields are air_embed_collect_t's, in its order, so one set of device arrays serves both
    shared = [f[0] for f in H.EmbedCollect._fields_ if f[0] in ("att", "run_digits", "gt_count", "gt_positions", "gt_boxes")]
    assert [f[0] for f in H.Localization._fields_][:5] == shared


def test_the_kernel_has_a_row_in_the_table_of_kernel_names(H):
    from air import air_model as am
    assert am.KERNEL_NAMES["air_localization"] == "loc_match_kernel"


def test_every_refusal_comes_before_a_launch(H):
    lib, ws = H.lib(), abi.host_ptr()
    call = lambda a, w=ws: lib.air_localization(C.byref(a), w, None)      # noqa: E731
    assert lib.air_localization(None, ws, None) == H.EINVAL
    for k in ("T", "B", "k", "G"):
        assert call(_desc(H, **{k: 0})) == H.EINVAL and call(_desc(H, **{k: -2})) == H.EINVAL, k
    assert call(_desc(H, k=65)) == H.EINVAL                                # k > B
    assert call(_desc(H, canvas_size=1)) == H.EINVAL and call(_desc(H, canvas_size=-50)) == H.EINVAL
    for tau in (0.0, -0.5, 1.0000001, float("nan"), float("inf"), -float("inf")):
        assert call(_desc(H, iou_threshold=tau)) == H.EINVAL, tau
    for missing in REQUIRED:
        assert call(_desc(H, **{missing: None})) == H.EINVAL, missing
    assert call(_desc(H), None) == H.EINVAL                                # no workspace
    assert call(_desc(H, match=None)) == H.EINVAL and call(_desc(H, iou=None)) == H.EINVAL      # exactly one of the two
    assert call(_desc(H, ptrs=False)) == H.EINVAL
    assert call(_desc(H, T=17)) == H.ELIMIT and call(_desc(H, G=17)) == H.ELIMIT
    # the order: a size before a limit, a limit before the canvas, the threshold and the pointers
    assert call(_desc(H, T=17, k=0)) == H.EINVAL and call(_desc(H, G=17, k=65)) == H.EINVAL
    assert call(_desc(H, ptrs=False, T=17)) == H.ELIMIT and call(_desc(H, G=17, iou_threshold=0.0)) == H.ELIMIT
    assert call(_desc(H, T=17, canvas_size=0), None) == H.ELIMIT


def test_workspace_query_answers_as_the_entry_point(H):
    q = H.lib().air_localization_workspace_bytes
    for T, B, k, G in ((1, 1, 1, 1), (3, 8, 5, 2), (16, 7, 7, 16), (3, 1000, 1000, 2), (3, 260, 256, 2), (3, 260, 257, 2)):
        assert q(T, B, k, G) == -(-k // lc.GROUP) * lc.SUMS * 8, (T, B, k, G)
    assert q(3, 2 ** 31 - 1, 2 ** 31 - 1, 2) == (2 ** 31 // 256) * 24    # no overflow at the largest batch
    for bad in ((0, 8, 8, 2), (3, 0, 0, 2), (3, 8, 0, 2), (3, 8, 8, 0), (3, 8, 9, 2), (-1, 8, 8, 2)):
        assert q(*bad) == H.EINVAL, bad
    assert q(17, 8, 8, 2) == H.ELIMIT and q(3, 8, 8, 17) == H.ELIMIT and q(16, 8, 8, 16) == 24
    assert q(17, 8, 9, 2) == H.EINVAL                                      # a size before a limit


def _stub(max_steps=3, batch_size=8, device_tensor=None):
    return types.SimpleNamespace(max_steps=max_steps, batch_size=batch_size, canvas_size=50,
                                 input_images=torch.zeros(batch_size, 2500) if device_tensor is None else device_tensor)


def test_python_class_refuses_on_the_host(H):
    from air.metrics import Localization
    assert Localization.names() == list(lc.NAMES)
    with pytest.raises(NotImplementedError, match="16"):
        Localization(_stub(max_steps=17), 2)
    with pytest.raises(NotImplementedError, match="holds 16 and 16"):
        Localization(_stub(), 17)
    with pytest.raises(ValueError, match="max_gt_digits"):
        Localization(_stub(), 0)
    for tau in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="iou_threshold"):
            Localization(_stub(), 2, iou_threshold=tau)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):           # valid arguments: what is missing is a device tensor
        Localization(_stub(), 2)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        Localization(_stub(device_tensor=np.zeros((8, 2500), np.float32)), 2)


def test_shift_order_is_the_permutation_of_the_images():
    import multi_mnist as mm
    rng = np.random.RandomState(3)
    for digits in (rng.randint(0, 3, 40), np.ones(7, np.int64), np.zeros(5, np.int64), np.asarray([1, 0, 2, 0])):
        images = np.arange(len(digits) * 3).reshape(len(digits), 3)
        order = mm.shift_zero_digits_order(digits)
        got_i, got_d = mm.shift_zero_digits_images(images, digits)
        assert np.array_equal(images[order], got_i) and np.array_equal(digits[order], got_d)
        assert sorted(order.tolist()) == list(range(len(digits)))


def test_generate_dataset_carries_the_ground_truth_through_the_shuffle():
    import multi_mnist as mm
    ds = mm.generate_dataset(max_digits=2, images_per_digit=12, test_set_size=10, seed=0)
    pos, box, digits = ds["test_positions"], ds["test_boxes"], ds["test_digits"]
    assert pos.shape == box.shape == (10, 2, 2) and pos.dtype == box.dtype == np.int32
    for i in range(10):
        canvas = ds["test_images"][i].reshape(50, 50)
        mask = np.zeros((50, 50), bool)
        for g in range(digits[i]):
            (x, y), (w, h) = pos[i, g], box[i, g]
            assert w > 0 and h > 0 and canvas[y:y + h, x:x + w].sum() > 0
            mask[y:y + h, x:x + w] = True
        assert canvas[~mask].sum() == 0                                      # all the ink lies inside the image's own boxes
        assert (pos[i, digits[i]:] == 0).all() and (box[i, digits[i]:] == 0).all()
    assert mm.padded_truth([[1, 2, 3, 4], []], [2, 0]).tolist() == [[[1, 2], [3, 4]], [[0, 0], [0, 0]]]
    assert mm.padded_truth([[], []], [0, 0]).shape == (2, 1, 2) and mm.padded_truth([[5, 6]], [1], 3).shape == (1, 3, 2)


def test_training_refuses_localization_on_a_cache_without_ground_truth(tmp_path):
    """parser.error (exit status 2) before anything touches a device or the results folder"""
    data = tmp_path / "multi_mnist_data"
    data.mkdir()
    for name in ("common.npz", "test.npz"):
        np.savez(str(data / name), images=np.zeros((4, 2500), np.float32), digits=np.zeros(4, np.int32))
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "training.py")
    p = subprocess.run([sys.executable, script, "--localization", "-r", str(tmp_path / "out")], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "holds none" in p.stderr and "multi_mnist.py" in p.stderr, (p.returncode, p.stderr[-400:])
    assert not (tmp_path / "out").exists()
    p = subprocess.run([sys.executable, script, "--localization", "--localization-iou", "0"], cwd=str(tmp_path),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--localization-iou" in p.stderr
