"""The scene source on the GPU (air_scene_source_compose / _advance, multi_mnist.DeviceSceneSource, training.py
--online-data) against the numpy restatement of tests/scene_source_cases.py -- bit for bit: every decision of the kernel is
integer arithmetic on Philox words and every canvas sum is exact.

The small cases use filled rectangles with a ragged edge and fractional ink, gd = 8, crop boxes of 4-7 pixels, on a
16 x 16 canvas: three of them leave little room, so second attempts and restarts happen in every batch of 256."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_source_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
GLYPHS = sc.ragged_glyphs()
CROPS = sc.crop_boxes(GLYPHS)
BIG = np.flatnonzero(CROPS[:, 2:].min(1) >= 5)                      # the glyphs whose box is 5-7 pixels both ways
KEYS = ("images", "digits", "indices", "positions", "boxes", "status")
GUARD = 64


def _bg(Cn, seed=3):
    return (np.random.RandomState(seed).randint(0, 9, size=(Cn, Cn)) / 16.0).astype(np.float32)


def _guarded(nbytes, dev):
    return torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)


def compose_raw(glyphs, crops, B, Cn, md, margin=0, gap=0, bg=None, counts=None, seed=0, max_attempts=100, max_restarts=32,
                batch=0, step_in_replay=0):
    """one launch through the C entry point into 0xFF-filled buffers with guard bytes behind each; -> dict of numpy outputs
    (the guards are checked here)"""
    from air import _hip as H
    dev = torch.device("cuda", 0)
    G, gd = glyphs.shape[0], glyphs.shape[1]
    t = lambda a, dt: torch.tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    g_d, c_d = t(glyphs.reshape(G, -1), torch.float32), t(crops, torch.int32)
    bg_d = None if bg is None else t(bg.reshape(-1), torch.float32)
    n_d = None if counts is None else t(counts, torch.int32)
    counter = torch.tensor([batch - step_in_replay], dtype=torch.int64, device=dev)
    sizes = dict(images=B * Cn * Cn * 4, digits=B * 4, indices=B * md * 4, positions=B * 2 * md * 4, boxes=B * 2 * md * 4,
                 status=B * 4)
    bufs = {k: _guarded(n, dev) for k, n in sizes.items()}
    a = H.SceneSource(g_d.data_ptr(), c_d.data_ptr(), H.ptr(bg_d), H.ptr(n_d), counter.data_ptr(),
                      *[bufs[k].data_ptr() for k in KEYS], None,
                      B, G, gd, Cn, margin, gap, md, max_attempts, max_restarts, seed)
    H.launch("air_scene_source_compose", dev, C.byref(a), step_in_replay)
    torch.cuda.synchronize()
    out = {}
    for k in KEYS:
        raw = bufs[k].cpu().numpy()
        assert (raw[sizes[k]:] == 0xFF).all(), "guard bytes behind %s" % k
        out[k] = raw[:sizes[k]].view(np.float32 if k == "images" else np.int32).reshape(B, -1)
    out["digits"], out["status"] = out["digits"].reshape(-1), out["status"].reshape(-1)
    return out


def assert_same(got, ref, rows=None):
    for k in KEYS:
        g, r = (got[k], ref[k]) if rows is None else (got[k][rows], ref[k][rows])
        assert g.dtype == r.dtype and np.array_equal(g, r), k


# ---------------------------------------------------------------------------------------------- 1. bit parity, roomy scenes
@pytest.mark.parametrize("given", [False, True], ids=["counts_drawn", "counts_given"])
@pytest.mark.parametrize("with_bg", [False, True], ids=["no_bg", "bg"])
@pytest.mark.parametrize("margin", [0, 1])
@pytest.mark.parametrize("gap", [0, 2])
def test_bit_parity_roomy_scenes(gap, margin, with_bg, given):
    B, Cn, md, seed = 256, 16, 3, 1000 + 16 * gap + 4 * margin + 2 * with_bg + given
    bg = _bg(Cn) if with_bg else None
    counts = (np.arange(B) % 4 if margin else np.full(B, 3)).astype(np.int32) if given else None
    kw = dict(margin=margin, gap=gap, bg=bg, counts=counts, seed=seed, max_attempts=100, max_restarts=32)
    ref = sc.compose_batch(B, 0, GLYPHS, CROPS, Cn, margin, gap, md, 100, 32, seed, counts, bg)
    got = compose_raw(GLYPHS, CROPS, B, Cn, md, **kw)
    print("gap %d margin %d: %d scenes restarted (most %d), %d gave up, digit counts %s" % (
        gap, margin, (ref["status"] > 0).sum(), ref["status"].max(), (ref["status"] < 0).sum(), np.bincount(ref["digits"], minlength=4)))
    assert_same(got, ref)
    # the retry and restart paths are part of what was compared, and nothing reached the bound
    assert (got["status"] > 0).any() and not (got["status"] == -1).any()
    if given:
        assert np.array_equal(got["digits"], counts)
    # every placed box keeps the margin (checked on the outputs themselves, not through the restatement)
    pos, box = got["positions"].reshape(B, md, 2), got["boxes"].reshape(B, md, 2)
    placed = np.arange(md)[None, :] < got["digits"][:, None]
    assert (box[placed] >= 4).all() and (pos[placed] >= margin).all() and ((pos + box)[placed] <= Cn - margin).all()


def test_bit_parity_odd_canvas_and_later_batches():
    """a 15 x 15 canvas (rows that are not 16-byte aligned: the 4-byte store path), gap 4 (the limit), batch indices behind
    2^32 wrap into the 32-bit counter word, and step_in_replay adds to the device counter"""
    B, Cn, md = 64, 15, 2
    bg = _bg(Cn)
    for batch, sir in ((7, 0), (7, 3), ((1 << 32) + 5, 1)):
        ref = sc.compose_batch(B, batch, GLYPHS, CROPS, Cn, 1, 4, md, 100, 32, 77, None, bg)
        got = compose_raw(GLYPHS, CROPS, B, Cn, md, margin=1, gap=4, bg=bg, seed=77, batch=batch, step_in_replay=sir)
        assert_same(got, ref)
    same = compose_raw(GLYPHS, CROPS, B, Cn, md, margin=1, gap=4, bg=bg, seed=77, batch=5)       # (uint32)(2^32 + 5) == 5
    assert_same(same, ref)


# --------------------------------------------------------------------------------------------------------- 2. the bound
@pytest.mark.parametrize("with_bg", [False, True], ids=["no_bg", "bg"])
def test_the_restart_bound_ends_the_scene(with_bg):
    """four digits of 5-7 pixels on 16 x 16 with two attempts each: most scenes restart and some never fit within 32 --
    those come back as an empty (or bg-only) canvas with digits 0 and status -1, a normal return; every other scene is the
    restatement's, and gave_up() counts them over the batches"""
    import multi_mnist as mm
    dev = torch.device("cuda", 0)
    B, Cn, md, seed = 256, 16, 4, 4242 + with_bg
    glyphs, crops = GLYPHS[BIG], CROPS[BIG]
    assert len(glyphs) >= 3 and crops[:, 2:].min() >= 5 and crops[:, 2:].max() <= 7
    bg = _bg(Cn) if with_bg else None
    counts = np.full(B, 4, np.int32)
    images, digits = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    src = mm.DeviceSceneSource(glyphs.reshape(len(glyphs), -1), B, images, digits, canvas_dim=Cn, max_digits=md, bg=bg,
                               counts=counts, seed=seed, max_attempts=2, max_restarts=32)
    total = 0
    for batch in range(2):
        src.next_batch()
        torch.cuda.synchronize()
        ref = sc.compose_batch(B, batch, glyphs, crops, Cn, 0, 0, md, 2, 32, seed, counts, bg)
        got = dict(images=images.cpu().numpy(), digits=digits.cpu().numpy(), **{k: v.cpu().numpy() for k, v in src.meta().items()})
        gone = got["status"] == -1
        print("batch %d: %d of %d scenes gave up, %d restarted" % (batch, gone.sum(), B, (got["status"] > 0).sum()))
        assert gone.any() and (~gone).any() and (got["status"] > 0).any()
        empty = np.zeros(Cn * Cn, np.float32) if bg is None else bg.reshape(-1)
        assert (got["images"][gone] == empty).all() and not got["digits"][gone].any()
        assert not got["indices"][gone].any() and not got["positions"][gone].any() and not got["boxes"][gone].any()
        assert (got["digits"][~gone] == 4).all()
        assert_same(got, ref)
        total += int(gone.sum())
        assert int(src.gave_up()) == total
    assert int(src.counter) == 2


# ------------------------------------------------------------------------------------------ 3. invariants at the model's shapes
def _check_invariants(got, glyphs, crops, Cn, md, margin, gap):
    B = len(got["digits"])
    assert (got["status"] >= 0).all()
    assert got["images"].min() >= 0.0 and got["images"].max() <= 1.0
    seen_two = False
    for b in range(B):
        n = int(got["digits"][b])
        assert 0 <= n <= md and n == int((got["boxes"][b].reshape(md, 2)[:, 0] > 0).sum())
        canvas, inks = np.zeros((Cn, Cn), np.float32), []
        for i in range(n):
            g, (x, y), (w, h) = got["indices"][b, i], got["positions"][b, 2 * i:2 * i + 2], got["boxes"][b, 2 * i:2 * i + 2]
            x0, y0, cw, ch = crops[g]
            assert (w, h) == (cw, ch)
            assert margin <= x and x + w <= Cn - margin and margin <= y and y + h <= Cn - margin
            crop = glyphs[g, y0:y0 + h, x0:x0 + w]
            canvas[y:y + h, x:x + w] += crop
            inks.append(np.argwhere(crop > 0) + (y, x))
        assert np.array_equal(canvas.reshape(-1), got["images"][b])            # the sum of its glyphs, exactly
        for i in range(n):
            for j in range(i):
                dist = np.abs(inks[i][:, None, :] - inks[j][None, :, :]).max(-1).min()
                assert dist > gap, (b, i, j, dist)                               # no shared ink pixel, none within the gap
                seen_two = True
        assert not got["indices"][b, n:].any() and not got["positions"][b, 2 * n:].any() and not got["boxes"][b, 2 * n:].any()
    assert seen_two


@pytest.fixture(scope="module")
def repo_glyphs():
    import multi_mnist as mm
    glyphs, _, _ = mm.load_glyphs()
    glyphs = glyphs[:400]
    return glyphs.reshape(len(glyphs), mm.IMAGE_SIZE, mm.IMAGE_SIZE), mm.crop_boxes(glyphs, mm.IMAGE_SIZE)


@pytest.mark.parametrize("B,Cn,md,margin,gap", [(64, 50, 2, 2, 1), (16, 128, 4, 1, 2)], ids=["50x50", "128x128"])
def test_invariants_at_the_models_shapes(repo_glyphs, B, Cn, md, margin, gap):
    glyphs, crops = repo_glyphs
    got = compose_raw(glyphs, crops, B, Cn, md, margin=margin, gap=gap, seed=9)
    if B >= 64:      # 64 uniform draws from 3 counts miss one with probability 3 (2/3)^64 < 1e-10; 16 from 5 do so in 13 %
        assert len(np.unique(got["digits"])) == md + 1                           # every count from 0 to max_digits occurs
    assert len(np.unique(got["digits"])) > 1
    _check_invariants(got, glyphs, crops, Cn, md, margin, gap)


# ---------------------------------------------------------------------------------------------- 4. determinism and sequence
def test_same_seed_same_bits_and_batches_differ():
    a = compose_raw(GLYPHS, CROPS, 64, 16, 3, gap=1, seed=5, batch=2)
    b = compose_raw(GLYPHS, CROPS, 64, 16, 3, gap=1, seed=5, batch=2)
    assert_same(a, b)
    nxt = compose_raw(GLYPHS, CROPS, 64, 16, 3, gap=1, seed=5, batch=3)
    other = compose_raw(GLYPHS, CROPS, 64, 16, 3, gap=1, seed=6, batch=2)
    assert not np.array_equal(a["images"], nxt["images"]) and not np.array_equal(a["positions"], nxt["positions"])
    assert not np.array_equal(a["images"], other["images"])


def test_replays_continue_the_eager_sequence():
    """three eager batches == the three batches of one 3-step AIRModel.capture_graph replay (the model's input buffer after
    each compose, copied out by the between_steps hook); a second replay goes on with batches 3-5"""
    import multi_mnist as mm
    from air import air_model as am
    from oracle import air_oracle as ao
    dev = torch.device("cuda", 0)
    hp = dict(ao.TRAINING_HP)
    B, Cn, md, steps, seed = 8, hp["canvas_size"], hp["max_digits"], 3, 31
    glyphs, _, _ = mm.load_glyphs()
    glyphs = glyphs[:200]
    crops = mm.crop_boxes(glyphs, mm.IMAGE_SIZE)

    ei, ed = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    eager = mm.DeviceSceneSource(glyphs, B, ei, ed, canvas_dim=Cn, max_digits=md, gap=1, seed=seed)
    want = []
    for _ in range(2 * steps):
        eager.next_batch()
        want.append((ei.clone(), ed.clone(), eager.meta()["positions"].clone()))
    torch.cuda.synchronize()
    ref0 = sc.compose_batch(B, 0, glyphs.reshape(-1, mm.IMAGE_SIZE, mm.IMAGE_SIZE), crops, Cn, 0, 1, md, 100, 32, seed)
    assert np.array_equal(want[0][0].cpu().numpy(), ref0["images"]) and np.array_equal(want[0][1].cpu().numpy(), ref0["digits"])

    am.reset_default_graph()
    images, targets = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    model = am.AIRModel(images, targets, cnn=False, train=True, scope="scene_source", gemm_precision="bf16", **hp)
    model.load_state_dict(ao.init_params(hp, 0))
    assert model.input_images is images
    piped = mm.DeviceSceneSource(glyphs, B, images, targets, canvas_dim=Cn, max_digits=md, gap=1, seed=seed)
    between, after = piped.graph_hooks(steps)
    assert after is None
    with pytest.raises(RuntimeError):
        piped.next_batch()
    with pytest.raises(ValueError):
        piped.graph_hooks(steps + 1)
    seen = [(torch.zeros_like(images), torch.zeros_like(targets), torch.zeros_like(piped.positions)) for _ in range(steps)]

    def hook(i):
        between(i)
        seen[i][0].copy_(model.input_images)
        seen[i][1].copy_(model.target_num_digits)
        seen[i][2].copy_(piped.positions)
    model.capture_graph(steps=steps, between_steps=hook)
    for rep in range(2):
        model.training()
        torch.cuda.synchronize()
        for i in range(steps):
            for got, ref in zip(seen[i], want[rep * steps + i]):
                assert torch.equal(got, ref), (rep, i)
    assert int(piped.counter) == 2 * steps == int(eager.counter)
    assert int(model.global_step) == 2 * steps and np.isfinite(float(model.loss))
    assert int(piped.gave_up()) == 0


# ------------------------------------------------------------------------------------------------------------- 5. driver
def _train(tmp_path, name, *flags):
    res = str(tmp_path / name)
    cmd = [sys.executable, "training.py", "-r", res, "-o", "1", "--iterations", "300", "--precision", "bf16"] + list(flags)
    p = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [json.loads(l) for l in open(os.path.join(res, "summary", "scalars.jsonl"))]
    for r in rows:
        r.pop("wall_s")
    final = re.search(r"test accuracy (\d\.\d+)  test loss (-?\d+\.\d+)  \(300 iterations", p.stdout)
    assert final, p.stdout[-1500:]
    return p.stdout, rows, final.groups(), res


def test_training_driver_online_data(tmp_path):
    """training.py --online-data --iterations 300 as 50-step replays and with --no-graph: both finish, report 0 canvases
    given up over 300 batches, and evaluate to the same numbers at every iteration both report (the test-set loss every 50
    iterations and at the end: the batches and the steps are the same bits either way).  Without the flag the driver says
    nothing about a source and leaves the layout it always left."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out_g, rows_g, final_g, _ = _train(tmp_path, "graph", "--online-data", "--print-every", "0", "--graph-steps", "50")
    out_e, rows_e, final_e, _ = _train(tmp_path, "eager", "--online-data", "--print-every", "50", "--no-graph")
    for out in (out_g, out_e):
        assert re.search(r"^online data: 300 batches composed on the device, 0 canvases given up$", out, flags=re.M), out[-1500:]
    assert [r["step"] for r in rows_g] == list(range(0, 300, 50))
    assert rows_g == rows_e and final_g == final_e
    losses = [r["loss"] for r in rows_g]
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]          # it trains on what the source makes
    lines = re.findall(r"^iteration (\d+)\tloss (-?\d+\.\d{3})\taccuracy (\d\.\d{2})$", out_e, flags=re.M)
    assert [int(l[0]) for l in lines] == list(range(50, 301, 50))
    out_p, rows_p, _, res = _train(tmp_path, "plain", "--print-every", "0")
    assert "online data" not in out_p
    assert [r["step"] for r in rows_p] == list(range(0, 300, 50)) and set(rows_p[0]) == set(rows_g[0])
    assert sorted(os.listdir(os.path.join(res, "models"))) == ["air-model-0.pt", "air-model-300.pt"]
    assert rows_p[0] == rows_g[0]                                                   # step 0: the same model on the same test set
