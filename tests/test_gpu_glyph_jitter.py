"""The glyph bank on the GPU (air_glyph_jitter, multi_mnist.DeviceGlyphBank, DeviceSceneSource on a bank, training.py
--online-data with jitter) against the numpy restatement of tests/glyph_jitter_cases.py -- bit for bit once the restatement
is given the kernel's own cos / sin, which in turn are within 4 * 2^-52 of scipy.special.cosdg / sindg -- and against what
scipy.ndimage itself makes of the same draws (tests/golden/glyph_jitter_scipy.npz: the GPU machine needs no scipy).

Shapes: gd = 8, od = 16, V = 256 variants of G = 12 glyphs (the ragged rectangles of the scene tests; the crowded case mixes
in four thin glyphs that a rotation can wipe out and squeezes the frames to od = 8, so that all three status values occur)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import glyph_jitter_cases as gj
import scene_source_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
KEYS = ("bank", "bank_crops", "source", "params", "status")
DTYPES = dict(bank=np.float32, bank_crops=np.int32, source=np.int32, params=np.float64, status=np.int32)
GUARD = 64


def jitter_raw(glyphs, crops, V, od, seed, generation, bounds, counter=True):
    """one launch through the C entry point into 0xFF-filled buffers with guard bytes behind each; -> dict of numpy outputs
    (the guards are checked here)"""
    from air import _hip as H
    dev = torch.device("cuda", 0)
    G, gd = glyphs.shape[0], glyphs.shape[1]
    g_d = torch.tensor(np.ascontiguousarray(glyphs.reshape(G, -1)), dtype=torch.float32, device=dev)
    c_d = torch.tensor(np.ascontiguousarray(crops), dtype=torch.int32, device=dev)
    n_d = torch.tensor([generation], dtype=torch.int64, device=dev) if counter else None
    sizes = dict(bank=V * od * od * 4, bank_crops=V * 16, source=V * 4, params=V * 48, status=V * 4)
    bufs = {k: torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    b = dict(gj.NEUTRAL, **bounds)
    a = H.GlyphJitter(g_d.data_ptr(), c_d.data_ptr(), H.ptr(n_d), *[bufs[k].data_ptr() for k in KEYS], V, G, gd, od,
                      b["min_w"], b["max_w"], b["min_h"], b["max_h"], b["min_ang"], b["max_ang"], seed)
    H.launch("air_glyph_jitter", dev, C.byref(a))
    torch.cuda.synchronize()
    out = {}
    for k in KEYS:
        raw = bufs[k].cpu().numpy()
        assert (raw[sizes[k]:] == 0xFF).all(), "guard bytes behind %s" % k
        out[k] = raw[:sizes[k]].view(DTYPES[k]).reshape(V, -1)
    out["source"], out["status"] = out["source"].reshape(-1), out["status"].reshape(-1)
    return out


def assert_same_bits(got, ref):
    assert np.array_equal(got["bank"].view(np.uint32), ref["bank"].view(np.uint32))
    for k in ("bank_crops", "source", "status"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["params"][:, :3].view(np.uint64), ref["params"][:, :3].view(np.uint64))
    assert not got["params"][:, 5].any()


@pytest.fixture(scope="module")
def launched():
    """every case of glyph_jitter_cases.GPU_CASES, launched once: name -> (outputs, the restatement fed the kernel's c, s)"""
    out = {}
    for name, (glyph_set, od, seed, generation, bounds) in gj.GPU_CASES.items():
        glyphs, crops = gj.gpu_glyphs(glyph_set)
        got = jitter_raw(glyphs, crops, gj.GPU_V, od, seed, generation, bounds)
        ref = gj.jitter_bank(glyphs, crops, gj.GPU_V, od, seed, generation, cs=got["params"][:, 3:5], **bounds)
        out[name] = (got, ref)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. bit parity
@pytest.mark.parametrize("name", list(gj.GPU_CASES))
def test_bit_parity(launched, name):
    got, ref = launched[name]
    _, od, seed, generation, bounds = gj.GPU_CASES[name]
    counts = np.bincount(ref["status"], minlength=3)
    print("%s: status counts %s, boxes up to %s" % (name, counts, got["bank_crops"][:, 2:].max(0)))
    assert_same_bits(got, ref)
    # cos / sin of the drawn angle (the fixture has cosdg / sindg of the restatement's angles, which are the kernel's bit
    # for bit: asserted above): both sides are within 2 ulp of values of magnitude <= 1
    want = np.load(os.path.join(ROOT, "tests", "golden", "glyph_jitter_scipy.npz"))[name + "_cs"]
    err = np.abs(got["params"][:, 3:5] - want).max()
    print("%s: |c - cosdg|, |s - sindg| <= %.3g (bound %.3g)" % (name, err, 4 * 2.0 ** -52))
    assert err <= 4 * 2.0 ** -52
    if name == "crowded":
        assert (counts > 0).all() and np.array_equal(np.bincount(got["status"], minlength=3), counts)
        bad = got["status"] != 0
        assert not got["bank"][bad].any() and not got["bank_crops"][bad].any()
    else:
        assert counts[0] == gj.GPU_V
    ok = got["status"] == 0
    assert (got["bank_crops"][ok][:, :2] == 0).all() and (got["bank_crops"][ok][:, 2:] >= 1).all()
    assert (got["bank_crops"][ok][:, 2:] <= od).all() and got["bank"].min() >= 0.0 and got["bank"].max() <= 1.0
    if "min_w" not in bounds:
        assert (got["params"][:, :2] == 1.0).all()
    if "min_ang" not in bounds:
        assert (got["params"][:, 2] == 0.0).all() and (got["params"][:, 3] == 1.0).all() and (got["params"][:, 4] == 0.0).all()


def test_generation_wraps_into_the_32_bit_counter_word_and_null_counter_is_zero(launched):
    glyph_set, od, seed, generation, bounds = gj.GPU_CASES["late"]
    assert generation > 1 << 32
    glyphs, crops = gj.gpu_glyphs(glyph_set)
    same = jitter_raw(glyphs, crops, gj.GPU_V, od, seed, generation & 0xFFFFFFFF, bounds)
    for k in KEYS:
        assert np.array_equal(same[k], launched["late"][0][k]), k
    zero = jitter_raw(glyphs, crops, 32, od, seed, 0, bounds)
    null = jitter_raw(glyphs, crops, 32, od, seed, 77, bounds, counter=False)
    for k in KEYS:
        assert np.array_equal(zero[k], null[k]), k


# ----------------------------------------------------------------------------------------------------- 2. the scipy fixture
@pytest.mark.parametrize("name", gj.FIXTURE_CASES)
def test_against_the_scipy_fixture(launched, name):
    """shapes equal for every variant; pixels equal or adjacent float32"""
    fx = np.load(os.path.join(ROOT, "tests", "golden", "glyph_jitter_scipy.npz"))
    shapes, pixels = fx[name + "_shapes"], fx[name + "_pixels"]
    got, _ = launched[name]
    od = gj.GPU_CASES[name][1]
    at = exact = 0
    for v in range(gj.GPU_V):
        h, w = (int(t) for t in shapes[v])
        if h == 0:
            assert got["status"][v] == 1, v
            continue
        assert got["status"][v] == 0 and tuple(got["bank_crops"][v]) == (0, 0, w, h), (v, got["bank_crops"][v], (h, w))
        mine, ref = got["bank"][v].reshape(od, od)[:h, :w], pixels[at:at + h * w].reshape(h, w)
        assert gj.adjacent_or_equal(mine, ref), v
        exact += np.array_equal(mine, ref)
        at += h * w
    assert at == len(pixels)
    print("%s: %d of %d variants equal scipy in every bit" % (name, exact, gj.GPU_V))


# -------------------------------------------------------------------------------------------------------- 3. determinism
def test_same_seed_and_generation_same_bank_next_generation_differs(launched):
    glyph_set, od, seed, generation, bounds = gj.GPU_CASES["both"]
    glyphs, crops = gj.gpu_glyphs(glyph_set)
    again = jitter_raw(glyphs, crops, gj.GPU_V, od, seed, generation, bounds)
    nxt = jitter_raw(glyphs, crops, gj.GPU_V, od, seed, generation + 1, bounds)
    other = jitter_raw(glyphs, crops, gj.GPU_V, od, seed + 1, generation, bounds)
    for k in KEYS:
        assert np.array_equal(again[k], launched["both"][0][k]), k
    for diff in (nxt, other):
        assert not np.array_equal(diff["bank"], again["bank"]) and not np.array_equal(diff["source"], again["source"])
        assert not np.array_equal(diff["params"][:, :3], again["params"][:, :3])


# ------------------------------------------------------------------------------------------------ 4. a scene source on a bank
def test_scene_source_on_a_bank():
    """16 x 16 canvas, three digits, gap 1, B = 256, from the crowded bank (od = 8: frames of 8 x 8, some variants unusable):
    the six outputs are the scene restatement's given the bank's own arrays; a scene whose first draw is an unusable variant
    restarts; none gives up; labels go through `source`"""
    import multi_mnist as mm
    dev = torch.device("cuda", 0)
    glyph_set, od, seed, _, bounds = gj.GPU_CASES["crowded"]
    glyphs, crops = gj.gpu_glyphs(glyph_set)
    B, Cn, md = 256, 16, 3
    bank = mm.DeviceGlyphBank(glyphs.reshape(len(glyphs), -1), gj.GPU_V, od=od, seed=seed, device=dev, **bounds)
    assert int(bank.status_counts()[0]) == 0                                   # nothing is usable before the first refresh
    bank.refresh()
    bank.refresh()                                                             # generation 1, the launched case's
    torch.cuda.synchronize()
    assert int(bank.counter) == 2
    ref_bank = gj.jitter_bank(glyphs, crops, gj.GPU_V, od, seed, 1, cs=bank.params[:, 3:5].cpu().numpy(), **bounds)
    assert np.array_equal(bank.bank.cpu().numpy(), ref_bank["bank"]) and np.array_equal(bank.status.cpu().numpy(), ref_bank["status"])
    counts = bank.status_counts().cpu().numpy()
    assert np.array_equal(counts, np.bincount(ref_bank["status"], minlength=3)) and (counts > 0).all()
    base_labels = np.arange(100, 100 + len(glyphs))
    assert np.array_equal(bank.labels(base_labels), base_labels[ref_bank["source"]])

    images, digits = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    given = np.full(B, md, np.int32)
    src = mm.DeviceSceneSource(bank, B, images, digits, canvas_dim=Cn, max_digits=md, gap=1, counts=given, seed=seed + 1)
    assert src.glyphs is bank.bank and src.crops is bank.bank_crops
    for batch in range(2):
        src.next_batch()                                                       # (does not refresh: the same bank twice)
        torch.cuda.synchronize()
        got = dict(images=images.cpu().numpy(), digits=digits.cpu().numpy(), **{k: v.cpu().numpy() for k, v in src.meta().items()})
        ref = sc.compose_batch(B, batch, ref_bank["bank"].reshape(gj.GPU_V, od, od), ref_bank["bank_crops"], Cn, 0, 1, md, 100,
                               32, seed + 1, given)
        for k in ("images", "digits", "indices", "positions", "boxes", "status"):
            assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), (batch, k)
        first = np.asarray([sc.Draws(b, batch, seed + 1).range(0, gj.GPU_V) for b in range(B)])
        hit = ref_bank["status"][first] != 0                                   # the scene's first glyph draw is unusable
        print("batch %d: %d scenes drew an unusable variant first, %d restarted, %d gave up" % (
            batch, hit.sum(), (got["status"] > 0).sum(), (got["status"] < 0).sum()))
        assert hit.sum() > 0 and (got["status"][hit] >= 1).all() and not (got["status"] < 0).any()
        placed = got["indices"][np.arange(md)[None, :] < got["digits"][:, None]]
        assert (ref_bank["status"][placed] == 0).all() and (got["digits"] == md).all()
    assert int(bank.counter) == 2 and int(src.gave_up()) == 0
    # "no glyph fits" is judged from the base crops and the smallest scale: 4 pixels at 0.9 leave 3, and 3 + 2 * 7 > 16
    ragged = sc.ragged_glyphs().reshape(12, -1)
    with pytest.raises(ValueError, match="no glyph fits"):
        mm.DeviceSceneSource(mm.DeviceGlyphBank(ragged, 16, od=16, device=dev, min_w=0.9), B, images, digits, canvas_dim=Cn,
                             max_digits=md, margin=7)
    mm.DeviceSceneSource(mm.DeviceGlyphBank(ragged, 16, od=16, device=dev, min_w=0.5, min_h=0.5), B, images, digits,
                         canvas_dim=Cn, max_digits=md, margin=7)


def test_compose_on_device_with_jitter():
    """multi_mnist.py --device N with jitter flags: a bank under the source, remade for every batch, labels through `source`"""
    import multi_mnist as mm
    _, base_labels, _ = mm.load_glyphs()
    kw = dict(max_digits=2, seed=3, batch_size=32, variants=256)
    out, _ = mm.compose_on_device(64, min_w=0.9, max_w=1.1, min_ang=-15.0, max_ang=15.0, **kw)
    plain, _ = mm.compose_on_device(64, **kw)                               # neutral: no bank, glyph indices as before
    assert out["images"].shape == (64, 2500) and (out["status"] >= 0).all() and (plain["status"] >= 0).all()
    used = np.arange(2)[None, :] < out["digits"][:, None]
    assert np.array_equal(out["digits"], plain["digits"])                   # (the scene draws are the source's, seed for seed)
    assert (out["indices"][used] < 256).all() and plain["indices"].max() >= 256
    assert np.array_equal(plain["labels"], np.where(used, base_labels[plain["indices"]], 0))
    assert set(np.unique(out["labels"][used])) <= set(np.unique(base_labels)) and not out["labels"][~used].any()
    assert not np.array_equal(out["images"], plain["images"]) and not np.array_equal(out["boxes"][:32], out["boxes"][32:])
    assert out["images"].min() >= 0.0 and out["images"].max() <= 1.0 and (out["images"].reshape(64, -1).any(1) == (out["digits"] > 0)).all()
    with pytest.raises(NotImplementedError, match="Generator.multi_image"):
        mm.compose_on_device(8, min_w=0.9, use_pixel_overlap=False)


# ----------------------------------------------------------------------------------------------------------------- 5. replay
def test_replays_refresh_the_bank_and_continue_the_eager_sequence():
    """two 3-step AIRModel.capture_graph replays, each with its own bank made by the replay's first launch, == the eager
    sequence refresh(); 3 x next_batch() twice, batch for batch"""
    import multi_mnist as mm
    from air import air_model as am
    from oracle import air_oracle as ao
    dev = torch.device("cuda", 0)
    hp = dict(ao.TRAINING_HP)
    B, Cn, md, steps, seed = 8, hp["canvas_size"], hp["max_digits"], 3, 41
    glyphs, _, _ = mm.load_glyphs()
    glyphs = glyphs[:200]
    jitter = dict(min_w=0.9, max_w=1.1, min_h=0.9, max_h=1.1, min_ang=-15.0, max_ang=15.0)

    ei, ed = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    ebank = mm.DeviceGlyphBank(glyphs, 128, seed=seed, device=dev, **jitter)
    eager = mm.DeviceSceneSource(ebank, B, ei, ed, canvas_dim=Cn, max_digits=md, gap=1, seed=seed)
    want, banks = [], []
    for rep in range(2):
        ebank.refresh()
        banks.append(ebank.bank.clone())
        for _ in range(steps):
            eager.next_batch()
            want.append((ei.clone(), ed.clone(), eager.meta()["indices"].clone(), eager.meta()["positions"].clone()))
    torch.cuda.synchronize()
    assert not torch.equal(banks[0], banks[1]) and int((ebank.status != 0).sum()) == 0
    assert any(int(w[1].sum()) > 0 for w in want)

    am.reset_default_graph()
    images, targets = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    model = am.AIRModel(images, targets, cnn=False, train=True, scope="glyph_bank", gemm_precision="bf16", **hp)
    model.load_state_dict(ao.init_params(hp, 0))
    pbank = mm.DeviceGlyphBank(glyphs, 128, seed=seed, device=dev, **jitter)
    piped = mm.DeviceSceneSource(pbank, B, images, targets, canvas_dim=Cn, max_digits=md, gap=1, seed=seed)
    between, after = piped.graph_hooks(steps)
    assert after is None
    seen = [(torch.zeros_like(images), torch.zeros_like(targets), torch.zeros_like(piped.indices), torch.zeros_like(piped.positions))
            for _ in range(steps)]

    def hook(i):
        between(i)
        seen[i][0].copy_(model.input_images)
        seen[i][1].copy_(model.target_num_digits)
        seen[i][2].copy_(piped.indices)
        seen[i][3].copy_(piped.positions)
    model.capture_graph(steps=steps, between_steps=hook)
    assert int(pbank.counter) == 0                                              # the capture made no bank
    for rep in range(2):
        model.training()
        torch.cuda.synchronize()
        assert torch.equal(pbank.bank, banks[rep]), rep
        for i in range(steps):
            for got, ref in zip(seen[i], want[rep * steps + i]):
                assert torch.equal(got, ref), (rep, i)
    assert int(pbank.counter) == 2 == int(ebank.counter) and int(piped.counter) == 2 * steps == int(eager.counter)
    assert int(model.global_step) == 2 * steps and np.isfinite(float(model.loss)) and int(piped.gave_up()) == 0


# ----------------------------------------------------------------------------------------------------------------- 6. driver
def _train(tmp_path, name, *flags):
    res = str(tmp_path / name)
    cmd = [sys.executable, "training.py", "-r", res, "-o", "1", "--iterations", "300", "--precision", "bf16", "--online-data",
           "--print-every", "0", "--min-width-scale", "0.9", "--max-width-scale", "1.1", "--min-height-scale", "0.9",
           "--max-height-scale", "1.1", "--min-rotation-angle", "-15", "--max-rotation-angle", "15"] + list(flags)
    p = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [json.loads(l) for l in open(os.path.join(res, "summary", "scalars.jsonl"))]
    for r in rows:
        r.pop("wall_s")
    final = re.search(r"test accuracy (\d\.\d+)  test loss (-?\d+\.\d+)  \(300 iterations", p.stdout)
    assert final, p.stdout[-1500:]
    return p.stdout, rows, final.groups()


def test_training_driver_online_data_with_jitter(tmp_path):
    """training.py --online-data --iterations 300 --print-every 0 with +-15 degrees and 0.9-1.1, as 50-step replays and with
    --no-graph: the same evaluation rows (six banks either way, made at the same steps), and a final line that counts the
    unusable variants"""
    out_g, rows_g, final_g = _train(tmp_path, "graph", "--graph-steps", "50")
    out_e, rows_e, final_e = _train(tmp_path, "eager", "--no-graph")
    line = r"^online data: 300 batches composed on the device, 0 canvases given up, 6 glyph banks of 4096 variants, (\d+) unusable in the last$"
    found = [re.search(line, out, flags=re.M) for out in (out_g, out_e)]
    assert all(found), (out_g[-800:], out_e[-800:])
    assert found[0].group(1) == found[1].group(1) and int(found[0].group(1)) < 4096
    assert [r["step"] for r in rows_g] == list(range(0, 300, 50))
    assert rows_g == rows_e and final_g == final_e
    losses = [r["loss"] for r in rows_g]
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]
