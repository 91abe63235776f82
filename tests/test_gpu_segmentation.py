"""GPU tests of the segmentation metrics (air_scene_masks, air_segmentation of include/air_hip.h, air/metrics.py).

The reference is the restatement of tests/segmentation_cases.py: labels in float32 in the header's order, the table in
integers, FG-ARI and mask IoU in float64 in the stated order, the sums by the stated tree.  Everything is compared BIT FOR
BIT.  Every buffer the kernels write is guarded: sentinels in front of and behind every output and the workspace, and behind
row k of the per-image outputs."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_check as abi
import segmentation_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 16                                   # sentinel elements in front of and behind every output (16: the planes stay aligned)
FILL_U8, FILL_I32, FILL_I64, FILL_F64 = 0xAB, -5, -(2 ** 40) - 5, -7.25
CASES = sc.gpu_cases()


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


FF = [False]                                 # True: the guarded buffers are filled with 0xFF bytes instead of the FILL_* values


class Guarded:
    """a device buffer of n elements between two rows of sentinels; `init` fills the payload"""

    def __init__(self, n, dtype, fill, init=None):
        self.n, self.fill, self.ff = n, fill, FF[0]
        if self.ff:
            size = torch.empty(0, dtype=dtype).element_size()
            self.buf = torch.full(((n + 2 * GUARD) * size,), 0xFF, dtype=torch.uint8, device="cuda").view(dtype)
        else:
            self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        if init is not None:
            self.buf[GUARD:GUARD + n] = init
        self.view = self.buf[GUARD:GUARD + n]

    def untouched(self, a):
        """whether every element of the numpy array `a` still is the fill"""
        return bool((a.view(np.uint8) == 0xFF).all()) if self.ff else bool((a == self.fill).all())

    def payload(self):
        """the payload as numpy, after checking the sentinels"""
        host = self.buf.cpu().numpy()
        assert self.untouched(host[:GUARD]) and self.untouched(host[GUARD + self.n:]), "a sentinel was overwritten"
        return host[GUARD:GUARD + self.n]


def run_case(H, case, outputs=True, upto=None, rows_behind=2):
    """the chunks of `case` through air_segmentation, one call each on shared accumulators, stream-ordered
    -> ([(pred_mask, tables, ari, mask_iou)] per chunk, counts, sums) as numpy; outputs=False passes the four as NULL"""
    T, B, G, Cc, w = case["T"], case["B"], case["G"], case["C"], case["w"]
    CC, cells = Cc * Cc, (G + 1) * (T + 1)
    counts = Guarded(sc.COUNTS, torch.int64, FILL_I64, init=0)
    sums = Guarded(sc.SUMS, torch.float64, FILL_F64, init=0.0)
    keep, outs = [], []
    for ch in case["chunks"][:upto]:
        k = ch["k"]
        nbytes = H.lib().air_segmentation_workspace_bytes(T, B, k, G)
        assert nbytes == k * sc.WORKSPACE_BYTES_PER_IMAGE
        ws = Guarded(nbytes // 8, torch.float64, FILL_F64)
        rows = k + rows_behind                           # the per-image outputs have rows beyond k, which must stay sentinels
        o = dict(pred_mask=Guarded(rows * CC, torch.uint8, FILL_U8), tables=Guarded(rows * cells, torch.int32, FILL_I32),
                 ari=Guarded(rows, torch.float64, FILL_F64), mask_iou=Guarded(rows * G, torch.float64, FILL_F64))
        d = {name: _dev(ch[name]) for name in ("att", "vrec", "gt_mask")}
        a = H.Segmentation(H.ptr(d["att"]), H.ptr(d["vrec"]), H.ptr(d["gt_mask"]),
                           *((H.ptr(o[n].view) if outputs else None) for n in ("pred_mask", "tables", "ari", "mask_iou")),
                           H.ptr(counts.view), H.ptr(sums.view), T, B, k, G, Cc, w, case["thr"])
        H.launch("air_segmentation", torch.device("cuda"), C.byref(a), H.ptr(ws.view))
        keep.append((d, ws))
        outs.append((o, k))
    torch.cuda.synchronize()
    for _, ws in keep:
        ws.payload()
    got = []
    for o, k in outs:
        row = []
        for name, per, shape in (("pred_mask", CC, (k, CC)), ("tables", cells, (k, G + 1, T + 1)), ("ari", 1, (k,)), ("mask_iou", G, (k, G))):
            v = o[name].payload()
            assert o[name].untouched(v[(k if outputs else 0) * per:]), "%s: a row >= k was written" % name
            row.append(v[:k * per].reshape(shape))
        got.append(tuple(row))
    return got, counts.payload(), sums.payload()


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bits = {1: np.uint8, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        bad = np.flatnonzero(np.ascontiguousarray(got).reshape(-1).view(bits) != np.ascontiguousarray(want).reshape(-1).view(bits))
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, bad.size, got.size, bad[:8].tolist(), got.reshape(-1)[bad[:8]].tolist(), want.reshape(-1)[bad[:8]].tolist()))


def check_case(H, name):
    case = CASES[name]
    want_out, want_c, want_s = sc.expected(name)
    got_out, got_c, got_s = run_case(H, case)
    print("%s: counts %s sums %s" % (name, got_c.tolist(), got_s.tolist()))
    for n, (got, want) in enumerate(zip(got_out, want_out)):
        for what, g, w_ in zip(("pred_mask", "tables", "ari", "mask_iou"), got, want):
            same_bits(g, w_, "%s chunk %d %s" % (name, n, what))
    same_bits(got_c, want_c, name + " counts")
    same_bits(got_s, want_s, name + " sums")
    return got_out, got_c, got_s


@pytest.mark.parametrize("name", [sc.shape_name(s) for s in sc.SHAPES])
def test_kernel_equals_the_restatement(H, name):
    """(T, G, k, B, C, w) = (1, 1, 1, 1, 8, 4); (2, 2, 3, 4, 16, 8); (3, 2, 5, 8, 15, 7): byte stores; (16, 16, 2, 2, 12, 6): the
    limits; (5, 4, 2, 2, 128, 32): the LDS grant; (3, 2, 257, 260, 10, 4): a second group in the tree"""
    check_case(H, name)


def test_every_branch_of_the_table(H):
    """overlapping windows, a window off the canvas, an inactive step between active ones, an exact tie, NaN window values,
    z_pres = 0, a pixel at the threshold, an unscored image -- tests/test_segmentation_cases.py asserts the table holds them"""
    got_out, got_c, _ = check_case(H, "branches")
    at, (pred, tables, ari, iou) = CASES["branches"]["planted"], got_out[0]
    assert 3 not in pred[at["tie"]] and 2 in pred[at["tie"]] and 2 not in pred[at["inactive_between"]]
    assert not pred[at["z_zero"]].any() and ari[at["z_zero"]] == 1.0 and np.isnan(ari[at["unscored"]])
    assert pred[at["at_threshold"]][0] == 0


def test_two_calls_accumulate(H):
    """two calls on the same accumulators = the restatement applied in the same two steps; the first call alone = its first
    step (so the second call added to what it found)"""
    check_case(H, "two_chunks")
    _, want_c, want_s = sc.expected("two_chunks", upto=1)
    _, got_c, got_s = run_case(H, CASES["two_chunks"], upto=1)
    assert got_c.tobytes() == want_c.tobytes() and got_s.tobytes() == want_s.tobytes()
    _, all_c, all_s = sc.expected("two_chunks")
    assert all_c[sc.IMAGES] == 8 and all_c.tobytes() != want_c.tobytes() and all_s.tobytes() != want_s.tobytes()


@pytest.mark.parametrize("name", ["branches", sc.shape_name(sc.SHAPES[5]), "two_chunks"])
def test_without_optional_outputs_the_accumulators_are_the_same(H, name):
    _, want_c, want_s = sc.expected(name)
    _, got_c, got_s = run_case(H, CASES[name], outputs=False)
    assert got_c.tobytes() == want_c.tobytes() and got_s.tobytes() == want_s.tobytes()


def test_the_same_inputs_give_the_same_bits(H):
    """twice, every output buffer filled with 0xFF bytes first: nothing of a previous content survives or matters"""
    FF[0] = True
    try:
        for name in (sc.shape_name(sc.SHAPES[5]), sc.shape_name(sc.SHAPES[1])):
            a, b = run_case(H, CASES[name]), run_case(H, CASES[name])
            want = sc.expected(name)
            for x in (a, b):
                for g, w_ in zip(x[0][0], want[0][0]):
                    assert g.tobytes() == w_.tobytes()
                assert x[1].tobytes() == want[1].tobytes() and x[2].tobytes() == want[2].tobytes()
    finally:
        FF[0] = False


def test_one_step_labels_are_the_render_canvas_above_the_threshold(H):
    """needs no restatement: with T = 1, z_pres = 1 and a canvas below 1, the label plane is air_render's canvas > threshold"""
    B, Cc, w, thr = 6, 20, 9, 0.375
    rng = np.random.RandomState(31)
    ch = sc.random_chunk(rng, 1, B, B, 1, Cc, w)
    ch["att"][:, :, sc.ATT_Z], ch["att"][:, :, sc.ATT_MASK] = 1.0, 1.0
    ch["vrec"] = rng.uniform(0.0, 0.9, ch["vrec"].shape).astype(np.float32)
    att, vrec, gt = _dev(ch["att"]), _dev(ch["vrec"]), _dev(ch["gt_mask"])
    canvas = torch.full((B, Cc * Cc), -1.0, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    r = H.Render(H.ptr(vrec), H.ptr(att), H.ptr(canvas), H.ptr(digits), B, 1, Cc, w)
    H.launch("air_render", torch.device("cuda"), C.byref(r))
    pred = torch.full((B, Cc * Cc), 9, dtype=torch.uint8, device="cuda")
    counts, sums = torch.zeros(sc.COUNTS, dtype=torch.int64, device="cuda"), torch.zeros(sc.SUMS, dtype=torch.float64, device="cuda")
    ws = torch.zeros(B * sc.WORKSPACE_BYTES_PER_IMAGE // 8, dtype=torch.float64, device="cuda")
    a = H.Segmentation(H.ptr(att), H.ptr(vrec), H.ptr(gt), H.ptr(pred), None, None, None, H.ptr(counts), H.ptr(sums),
                       1, B, B, 1, Cc, w, thr)
    H.launch("air_segmentation", torch.device("cuda"), C.byref(a), H.ptr(ws))
    torch.cuda.synchronize()
    assert float(canvas.max()) < 1.0 and float(canvas.min()) >= 0.0
    want = (canvas > thr).to(torch.uint8)
    assert 0 < int(want.sum()) < want.numel() and torch.equal(pred, want)


def test_scene_masks_on_hand_placed_glyphs_and_on_a_scene_source_batch(H):
    """air_scene_masks against numpy: the hand-placed scenes (intersecting boxes, the smallest digit wins, unusable slots),
    then a DeviceSceneSource batch (16 x 16, three digits, gap 0), where the labels must also cover exactly the ink"""
    import multi_mnist as mm
    from air.metrics import Segmentation
    s = sc.hand_scene()
    arrays = {k: _dev(s[k]) for k in ("glyphs", "crops", "indices", "positions")}
    for thr in (0.0, 0.75):
        got = Segmentation.scene_masks(dict(arrays, canvas_dim=s["C"]), _dev(s["digits"]), ink_threshold=thr)
        want = sc.scene_masks(s["glyphs"], s["crops"], s["digits"], s["indices"], s["positions"], s["C"], thr)
        assert got.dtype == torch.uint8 and got.cpu().numpy().tobytes() == want.tobytes()
    B, Cn, md = 64, 16, 3
    import scene_source_cases as ssc
    glyphs = ssc.ragged_glyphs().reshape(12, 64)                 # rectangles of 4 .. 7 pixels in 8 x 8 frames, ragged edges
    images = torch.zeros(B, Cn * Cn, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    source = mm.DeviceSceneSource(glyphs, B, images, digits, canvas_dim=Cn, max_digits=md, gap=0, seed=11)
    source.next_batch()
    got = Segmentation.scene_masks(source, digits)
    meta = source.meta()
    want = sc.scene_masks(source.glyphs.cpu().numpy(), source.crops.cpu().numpy(), digits.cpu().numpy(),
                          meta["indices"].cpu().numpy(), meta["positions"].cpu().numpy(), Cn)
    got = got.cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert ((got > 0) == (images.cpu().numpy() > 0)).all()                   # no bg: the labels cover exactly the ink
    assert int(digits.max()) == md and set(np.unique(got).tolist()) == set(range(md + 1))
    # a guarded mask whose plane is not 16-byte aligned and an odd canvas: the byte path, nothing outside
    s15 = Guarded(2 * 15 * 15, torch.uint8, FILL_U8)
    view = s15.buf[GUARD + 1:GUARD + 1 + 2 * 225]
    a = H.SceneMasks(H.ptr(arrays["glyphs"]), H.ptr(arrays["crops"]), H.ptr(_dev(s["digits"])), H.ptr(arrays["indices"]),
                     H.ptr(arrays["positions"]), H.ptr(view), 2, 4, s["gd"], 15, 4, 0.0)
    H.launch("air_scene_masks", torch.device("cuda"), C.byref(a))
    torch.cuda.synchronize()
    host = s15.buf.cpu().numpy()
    want15 = sc.scene_masks(s["glyphs"], s["crops"], s["digits"], s["indices"], s["positions"], 15)
    assert (host[:GUARD + 1] == FILL_U8).all() and (host[GUARD + 1 + 450:] == FILL_U8).all()
    assert host[GUARD + 1:GUARD + 451].tobytes() == want15.tobytes()


# -------------------------------------------------------------------------------------------------------------- the module
def test_module_on_a_real_model_and_a_scene_source(H):
    """AIRModel(cnn=False, train=False) at B = 8, T = 3 on scenes a DeviceSceneSource composed into its input buffer, masks
    from scene_masks.  Accumulators, kept outputs and values() equal the restatement on the model's records and windows copied
    to the host.  (The z_pres bias of a fresh model is raised until it infers objects.)"""
    import multi_mnist as mm
    from air import air_model as am
    from air.metrics import Segmentation
    from oracle import air_oracle as ao
    hp = dict(ao.TRAINING_HP)
    B, T, G, Cc, w = 8, hp["max_steps"], 2, hp["canvas_size"], hp["windows_size"]
    am.reset_default_graph()
    images = torch.zeros(B, Cc ** 2, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    model = am.AIRModel(images, digits, cnn=False, train=False, scope="seg8", gemm_precision="fp32", **hp)
    params = {k: np.array(v) for k, v in ao.init_params(hp, 0).items()}
    bias = "z_pres/log_odds/output/biases"
    source = mm.DeviceSceneSource(mm.load_glyphs()[0], B, images, digits, canvas_dim=Cc, max_digits=G, seed=5)
    source.next_batch()
    for raised in range(12):
        model.load_state_dict(params)
        model.forward()
        if int(model.run_digits.sum()) >= 4:
            break
        params[bias] = params[bias] + np.float32(1.0)
    masks = Segmentation.scene_masks(source, digits)
    assert tuple(masks.shape) == (B, Cc * Cc) and ((masks > 0) == (images > 0)).all()
    thr = 0.25
    seg = Segmentation(model, G, pred_threshold=thr, keep=True)
    assert seg.names() == list(sc.NAMES)
    seg.update(masks)
    values = seg.values()
    assert values.is_cuda and values.dtype == torch.float64
    case = dict(T=T, B=B, G=G, C=Cc, w=w, thr=thr)
    chunk = dict(k=B, att=model.att.cpu().numpy(), vrec=model.vrec.cpu().numpy(), gt_mask=masks.cpu().numpy())
    counts, sums = sc.empty_accumulators()
    pred, tables, ari, iou = sc.apply_chunk(case, chunk, counts, sums)
    print("real model (z_pres bias raised %d times): counts %s sums %s" % (raised, counts.tolist(), sums.tolist()))
    assert counts[sc.PRESENT] > 0 and counts[sc.FG_PIXELS] > 0
    same_bits(seg.pred_mask.cpu().numpy(), pred, "pred_mask")
    same_bits(seg.tables.cpu().numpy(), tables, "tables")
    same_bits(seg.ari.cpu().numpy(), ari, "ari")
    same_bits(seg.mask_iou.cpu().numpy(), iou, "mask_iou")
    same_bits(seg.counts.cpu().numpy(), counts, "counts")
    same_bits(seg.sums.cpu().numpy(), sums, "sums")
    assert values.cpu().numpy().tobytes() == sc.derived(counts, sums, Cc).tobytes()
    res = seg.result()
    assert [res[n] for n in sc.NAMES] == [v if v == v else res[n] for n, v in zip(sc.NAMES, sc.derived(counts, sums, Cc).tolist())]
    assert res["images"] == B and res["fg_pixels"] == int(counts[sc.FG_PIXELS])
    # a second update adds; reset() and k < B with the [k, C, C] form of the planes
    seg.update(masks)
    assert int(seg.counts[sc.IMAGES]) == 2 * B
    seg.reset()
    assert np.isnan(seg.values().cpu().numpy()).all()
    seg.update(masks.view(B, Cc, Cc), k=5)
    c5, s5 = sc.empty_accumulators()
    sc.apply_chunk(case, dict(chunk, k=5), c5, s5)
    same_bits(seg.counts.cpu().numpy(), c5, "counts, k = 5")
    same_bits(seg.sums.cpu().numpy(), s5, "sums, k = 5")
    with pytest.raises(ValueError):
        seg.update(masks, k=B + 1)
    with pytest.raises(ValueError):
        seg.update(masks[:, :100].contiguous())
    with pytest.raises(ValueError):
        seg.update(masks.int())
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        seg.update(masks.cpu())
    # the picture: labels in the colours of the boxes
    from air.visualize import colour_masks
    rgb = colour_masks(seg.pred_mask, images)
    assert tuple(rgb.shape) == (B, Cc, Cc, 3) and float(rgb.max()) <= 1.0 and float(rgb.min()) >= 0.0


def test_driver_hundred_iterations_with_the_flag(H, tmp_path):
    """training.py --segmentation for 100 iterations on a device-composed test set: the rows of scalars.jsonl carry the seg_*
    keys (numbers or null) beside the usual ones"""
    script = os.path.join(abi.ROOT, "tf-attend-infer-repeat_amd", "training.py")
    out = tmp_path / "run"
    p = subprocess.run([sys.executable, script, "--online-data", "--glyph-style", "mnist-like", "--segmentation", "--iterations", "100", "--print-every", "0",
                        "--jitter-bank", "256", "-r", str(out)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-600:], p.stderr[-1200:])
    rows = [json.loads(ln) for ln in open(out / "summary" / "scalars.jsonl")]
    assert [r["step"] for r in rows] == [0, 50]
    for r in rows:
        assert {"seg_fg_ari", "seg_mask_iou", "seg_fg_missed", "seg_bg_claimed"} <= set(r) and "loc_mean_iou" not in r
        assert r["seg_fg_missed"] is not None and 0.0 <= r["seg_fg_missed"] <= 1.0 and 0.0 <= r["seg_bg_claimed"] <= 1.0
        assert r["seg_mask_iou"] is not None and 0.0 <= r["seg_mask_iou"] <= 1.0
    assert "segmentation at 0.5:" in p.stdout
