"""The handwriting bank on the GPU (air_glyph_distort, multi_mnist.DeviceHandwritingBank, DeviceSceneSource on such a bank,
training.py --online-data --glyph-style mnist-like) against the numpy restatement of tests/glyph_distort_cases.py -- bit for
bit once the restatement is given the kernel's own cos / sin, which in turn are within 4 * 2^-52 of scipy.special.cosdg /
sindg (tests/golden/glyph_distort_cs.npz).

Shapes: V = 256 variants at the smallest planes where each stage can go wrong -- glyph_distort_cases.GPU_CASES says which."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import glyph_distort_cases as gd
import scene_source_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
KEYS = ("bank", "bank_crops", "source", "params", "status")
DTYPES = dict(bank=np.float32, bank_crops=np.int32, source=np.int32, params=np.float64, status=np.int32)
GUARD = 64


def distort_raw(glyphs, V, od, ink, seed, generation, radius, bounds, counter=True):
    """one launch through the C entry point into 0xFF-filled buffers with guard bytes behind each; -> dict of numpy outputs
    (the guards are checked here)"""
    from air import _hip as H
    dev = torch.device("cuda", 0)
    G, gdim = glyphs.shape[0], glyphs.shape[1]
    b = dict(gd.NEUTRAL, **bounds)
    taps, R = gd.gaussian_taps(b["sigma"], radius)
    g_d = torch.tensor(np.ascontiguousarray(glyphs.reshape(G, -1)), dtype=torch.float32, device=dev)
    t_d = torch.tensor(taps, dtype=torch.float64, device=dev)
    n_d = torch.tensor([generation], dtype=torch.int64, device=dev) if counter else None
    sizes = dict(bank=V * od * od * 4, bank_crops=V * 16, source=V * 4, params=V * 64, status=V * 4)
    bufs = {k: torch.full((n + GUARD,), 0xFF, dtype=torch.uint8, device=dev) for k, n in sizes.items()}
    a = H.GlyphDistort(g_d.data_ptr(), H.ptr(n_d), t_d.data_ptr(), *[bufs[k].data_ptr() for k in KEYS], V, G, gdim, od, ink, R,
                       b["min_stroke"], b["max_stroke"], gd.field_gain(taps, b["alpha"]), b["max_ang"], b["max_shear"],
                       b["min_scale"], b["max_scale"], b["lo"], b["hi"], seed)
    H.launch("air_glyph_distort", dev, C.byref(a))
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
    cols = [0, 1, 2, 3, 6, 7]                                                    # all but c, s
    assert np.array_equal(got["params"][:, cols].view(np.uint64), ref["params"][:, cols].view(np.uint64))


def _launch(name, **override):
    glyph_set, gdim, od, ink, seed, generation, radius, bounds = gd.GPU_CASES[name]
    kw = dict(V=gd.GPU_V, od=od, ink=ink, seed=seed, generation=generation, radius=radius, bounds=bounds)
    kw.update(override)
    return distort_raw(gd.gpu_glyphs(glyph_set, gdim), **kw)


@pytest.fixture(scope="module")
def launched():
    """every case of glyph_distort_cases.GPU_CASES, launched once: name -> (outputs, the restatement fed the kernel's c, s)"""
    out = {}
    for name, (glyph_set, gdim, od, ink, seed, generation, radius, bounds) in gd.GPU_CASES.items():
        got = _launch(name)
        ref = gd.distort_bank(gd.gpu_glyphs(glyph_set, gdim), gd.GPU_V, od, ink, seed, generation, cs=got["params"][:, 4:6],
                              radius=radius, **bounds)
        out[name] = (got, ref)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. bit parity
@pytest.mark.parametrize("name", list(gd.GPU_CASES))
def test_bit_parity(launched, name):
    got, ref = launched[name]
    glyph_set, gdim, od, ink, seed, generation, radius, bounds = gd.GPU_CASES[name]
    counts = np.bincount(ref["status"], minlength=3)
    ok = got["status"] == 0
    print("%s: status counts %s, boxes %s .. %s, fit factors %.3g .. %.3g" % (
        name, counts, got["bank_crops"][ok][:, 2:].min(0), got["bank_crops"][ok][:, 2:].max(0),
        got["params"][ok][:, 7].min(), got["params"][ok][:, 7].max()))
    assert_same_bits(got, ref)
    # cos / sin of the drawn angle (the fixture has cosdg / sindg of the restatement's angles, which are the kernel's bit
    # for bit: asserted above): both sides are within 2 ulp of values of magnitude <= 1
    want = np.load(os.path.join(ROOT, "tests", "golden", "glyph_distort_cs.npz"))[name + "_cs"]
    err = np.abs(got["params"][:, 4:6] - want).max()
    print("%s: |c - cosdg|, |s - sindg| <= %.3g (bound %.3g)" % (name, err, 4 * 2.0 ** -52))
    assert err <= 4 * 2.0 ** -52
    # what every bank holds
    assert ok.sum() > 0 and counts[2] == 0
    crops = got["bank_crops"][ok]
    assert (crops[:, :2] >= 0).all() and (crops[:, 2:] >= 1).all() and (crops[:, 0] + crops[:, 2] <= od).all()
    assert (crops[:, 1] + crops[:, 3] <= od).all() and (crops[:, 2:].max(1) <= ink).all()
    assert not got["bank"][~ok].any() and not got["bank_crops"][~ok].any()
    assert got["bank"].min() >= 0.0 and got["bank"].max() <= 1.0 and not np.signbit(got["bank"]).any()
    b = dict(gd.NEUTRAL, **bounds)
    if b["max_ang"] == 0.0:
        assert (got["params"][:, 0] == 0.0).all() and (got["params"][:, 4] == 1.0).all() and (got["params"][:, 5] == 0.0).all()
    if b["max_shear"] == 0.0:
        assert (got["params"][:, 1] == 0.0).all()
    if b["min_scale"] == 1.0 and b["max_scale"] == 1.0:
        assert (got["params"][:, 2:4] == 1.0).all()
    assert got["params"][:, 6].min() >= b["min_stroke"] and got["params"][:, 6].max() <= b["max_stroke"]
    # what the case is there for
    f = got["params"][ok][:, 7]
    if name == "small":
        assert radius >= gdim and (gdim, od, ink) == (8, 16, 10) and f.min() > 1.0     # a tap line wider than the plane
    if name == "preset":
        assert (gdim, od, ink) == (24, 28, 20) and bounds == gd.MNIST_LIKE and set(got["params"][:, 6]) == {-1.0, 0.0, 1.0}
    if name in ("preset", "thick"):
        assert f.min() < 1.0 < f.max()                                           # boxes are both enlarged and reduced
    if name == "thin":
        assert counts[1] > 0 and counts[0] > 0 and (got["params"][:, 6] == -2.0).all()
        assert set(got["source"][ok]) == {6}                                     # only the block survives two erosions
    if name == "thick":
        assert counts[0] == gd.GPU_V and (got["params"][:, 6] == 2.0).all()
    if name == "one_tap":
        assert radius == 0
    if name == "lines":
        ones = (crops[:, 2:] == 1).any(1)
        assert ones.sum() > 0 and counts[0] == gd.GPU_V                           # 1 x k and k x 1 boxes come out usable
    if name == "clamped":
        assert od == ink and ((crops[:, 0] == 0) | (crops[:, 1] == 0)).all()     # the larger side fills the frame


def test_generation_wraps_into_the_32_bit_counter_word_and_null_counter_is_zero(launched):
    generation = gd.GPU_CASES["late"][5]
    assert generation > 1 << 32
    same = _launch("late", generation=generation & 0xFFFFFFFF)
    for k in KEYS:
        assert np.array_equal(same[k], launched["late"][0][k]), k
    zero = _launch("late", V=32, generation=0)
    null = _launch("late", V=32, generation=77, counter=False)
    for k in KEYS:
        assert np.array_equal(zero[k], null[k]), k
    assert not np.array_equal(zero["bank"], same["bank"][:32])


# -------------------------------------------------------------------------------------------------------- 2. determinism
def test_same_seed_and_generation_same_bank_next_generation_differs(launched):
    seed, generation = gd.GPU_CASES["preset"][4:6]
    again = _launch("preset")
    nxt = _launch("preset", generation=generation + 1)
    other = _launch("preset", seed=seed + 1)
    for k in KEYS:
        assert np.array_equal(again[k], launched["preset"][0][k]), k
    for diff in (nxt, other):
        assert not np.array_equal(diff["bank"], again["bank"]) and not np.array_equal(diff["source"], again["source"])
        assert not np.array_equal(diff["params"][:, :4], again["params"][:, :4])


# --------------------------------------------------------------------------------------------- 3. the class, a scene source
def test_bank_class_and_a_scene_source_on_it():
    """DeviceHandwritingBank of the preset on its own base glyphs (40 -> 20 in 28; the host-made taps and gain) equals the
    restatement; a scene source on it equals the scene restatement given the bank's arrays; labels go through `source`"""
    import multi_mnist as mm
    dev = torch.device("cuda", 0)
    p = dict(mm.MNIST_LIKE)
    side, ink, od = p.pop("side"), p.pop("ink"), p.pop("od")
    base, base_labels = mm.load_base_glyphs(side)
    base, base_labels = base[:300], base_labels[:300]
    V, B, Cn, md, seed = 128, 64, 50, 2, 77
    bank = mm.DeviceHandwritingBank(base, V, od=od, ink=ink, seed=seed, device=dev, **p)
    assert int(bank.status_counts()[0]) == 0                                   # nothing is usable before the first refresh
    bank.refresh()
    bank.refresh()
    torch.cuda.synchronize()
    assert int(bank.counter) == 2 and bank.radius == 24 and bank.params.shape == (V, 8)
    ref = gd.distort_bank(base.reshape(-1, side, side), V, od, ink, seed, 1, cs=bank.params[:, 4:6].cpu().numpy(), **p)
    got = {k: getattr(bank, k).cpu().numpy() for k in KEYS}
    assert_same_bits(got, ref)
    counts = bank.status_counts().cpu().numpy()
    assert np.array_equal(counts, np.bincount(ref["status"], minlength=3)) and counts[0] >= V - 4
    assert np.array_equal(bank.labels(base_labels), base_labels[ref["source"]])
    assert bank.fits(Cn, 0) and bank.fits(20, 0) and not bank.fits(20, 1)

    images, digits = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    src = mm.DeviceSceneSource(bank, B, images, digits, canvas_dim=Cn, max_digits=md, gap=1, seed=seed + 1)
    assert src.glyphs is bank.bank and src.crops is bank.bank_crops and src.bank is bank
    for batch in range(2):
        src.next_batch()                                                       # (does not refresh: the same bank twice)
        torch.cuda.synchronize()
        out = dict(images=images.cpu().numpy(), digits=digits.cpu().numpy(), **{k: v.cpu().numpy() for k, v in src.meta().items()})
        want = sc.compose_batch(B, batch, ref["bank"].reshape(V, od, od), ref["bank_crops"], Cn, 0, 1, md, 100, 32, seed + 1)
        for k in ("images", "digits", "indices", "positions", "boxes", "status"):
            assert out[k].dtype == want[k].dtype and np.array_equal(out[k], want[k]), (batch, k)
        assert (out["status"] >= 0).all() and out["digits"].max() == md
    assert int(bank.counter) == 2 and int(src.gave_up()) == 0
    with pytest.raises(ValueError, match="no glyph fits"):
        mm.DeviceSceneSource(bank, B, images, digits, canvas_dim=Cn, max_digits=md, margin=16)


def test_compose_on_device_mnist_like():
    """multi_mnist.py --device N --glyph-style mnist-like: a handwriting bank under the source, remade for every batch"""
    import multi_mnist as mm
    _, base_labels = mm.load_base_glyphs()
    kw = dict(max_digits=2, seed=3, batch_size=32, variants=128)
    out, source = mm.compose_on_device(64, glyph_style="mnist-like", **kw)
    plain, _ = mm.compose_on_device(64, **kw)
    assert "mnist-like" in source and out["images"].shape == (64, 2500) and (out["status"] >= 0).all()
    used = np.arange(2)[None, :] < out["digits"][:, None]
    assert np.array_equal(out["digits"], plain["digits"])                   # (the scene draws are the source's, seed for seed)
    assert (out["indices"][used] < 128).all()
    sides = out["boxes"].reshape(64, 2, 2).max(2)[used]                     # MNIST's 20-pixel box (the fit's second threshold
    assert (sides <= 20).all() and (sides == 20).mean() > 0.9               # empties an edge row of 1 variant in ~2 000)
    assert set(np.unique(out["labels"][used])) <= set(np.unique(base_labels)) and not out["labels"][~used].any()
    assert not np.array_equal(out["boxes"][:32], out["boxes"][32:])
    assert out["images"].min() >= 0.0 and out["images"].max() <= 1.0 and (out["images"].any(1) == (out["digits"] > 0)).all()
    with pytest.raises(ValueError, match="mnist-like"):
        mm.compose_on_device(8, glyph_style="mnist-like", min_w=0.9)


# ----------------------------------------------------------------------------------------------------------------- 4. replay
def test_replays_refresh_the_bank_and_continue_the_eager_sequence():
    """two 3-step AIRModel.capture_graph replays, each with its own bank made by the replay's first launch, == the eager
    sequence refresh(); 3 x next_batch() twice, batch for batch"""
    import multi_mnist as mm
    from air import air_model as am
    from oracle import air_oracle as ao
    dev = torch.device("cuda", 0)
    hp = dict(ao.TRAINING_HP)
    B, Cn, md, steps, seed = 8, hp["canvas_size"], hp["max_digits"], 3, 43

    ei, ed = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    ebank, _ = mm.handwriting_bank(128, seed, dev)
    eager = mm.DeviceSceneSource(ebank, B, ei, ed, canvas_dim=Cn, max_digits=md, gap=1, seed=seed)
    want, banks = [], []
    for rep in range(2):
        ebank.refresh()
        banks.append(ebank.bank.clone())
        for _ in range(steps):
            eager.next_batch()
            want.append((ei.clone(), ed.clone(), eager.meta()["indices"].clone(), eager.meta()["positions"].clone()))
    torch.cuda.synchronize()
    assert not torch.equal(banks[0], banks[1]) and any(int(w[1].sum()) > 0 for w in want)

    am.reset_default_graph()
    images, targets = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    model = am.AIRModel(images, targets, cnn=False, train=True, scope="handwriting_bank", gemm_precision="bf16", **hp)
    model.load_state_dict(ao.init_params(hp, 0))
    pbank, _ = mm.handwriting_bank(128, seed, dev)
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


# ----------------------------------------------------------------------------------------------------------------- 5. driver
def _train(tmp_path, name, *flags):
    res = str(tmp_path / name)
    cmd = [sys.executable, "training.py", "-r", res, "-o", "1", "--iterations", "300", "--precision", "bf16", "--online-data",
           "--print-every", "0", "--glyph-style", "mnist-like", "--jitter-bank", "1024"] + list(flags)
    p = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [json.loads(l) for l in open(os.path.join(res, "summary", "scalars.jsonl"))]
    for r in rows:
        r.pop("wall_s")
    final = re.search(r"test accuracy (\d\.\d+)  test loss (-?\d+\.\d+)  \(300 iterations", p.stdout)
    assert final, p.stdout[-1500:]
    return p.stdout, rows, final.groups()


def test_training_driver_online_data_mnist_like(tmp_path):
    """training.py --online-data --glyph-style mnist-like --iterations 300 --print-every 0, as 50-step replays and with
    --no-graph: the same evaluation rows (six banks either way, made at the same steps, the same device-made test set), a
    final line that counts the banks, and no host generator"""
    out_g, rows_g, final_g = _train(tmp_path, "graph", "--graph-steps", "50")
    out_e, rows_e, final_e = _train(tmp_path, "eager", "--no-graph")
    line = r"^online data: 300 batches composed on the device, 0 canvases given up, 6 glyph banks of 1024 variants, (\d+) unusable in the last$"
    found = [re.search(line, out, flags=re.M) for out in (out_g, out_e)]
    assert all(found), (out_g[-800:], out_e[-800:])
    assert found[0].group(1) == found[1].group(1) and int(found[0].group(1)) < 64
    assert "Generating multi-digit dataset" not in out_g and "Generating multi-digit dataset" not in out_e
    assert [r["step"] for r in rows_g] == list(range(0, 300, 50))
    assert rows_g == rows_e and final_g == final_e
    losses = [r["loss"] for r in rows_g]
    assert all(np.isfinite(v) for v in losses) and losses[-1] < losses[0]
