"""GPU tests of the histogram summaries (air_histograms, include/air_hip.h; AIRModel.var_summaries / grad_summaries;
training.py --tensorboard).

The reference is the numpy restatement of TensorFlow 1.3's histogram below: the limits from the double loop, the bucket of a
value np.searchsorted(limits, float64(x), side="right"), the sums in float64.  Counts, num, min and max are compared exactly;
sum and sum_squares within n * 2^-53 * sum|x| (|x|^2) of the EXACT sum (math.fsum; numpy's float64 sum where n is large and
its own error, ~log2(n) * 2^-53, is far inside the bound): the error bound of any order of n - 1 float64 additions plus the
rounding of the exact sum itself -- no tuned tolerance."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_check as abi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
GUARD = 64                                             # bytes behind every output / workspace buffer


def _limits():
    pos, v = [], 1e-12
    while v < 1e20:
        pos.append(v)
        v *= 1.1
    pos.append(sys.float_info.max)
    return np.array([-x for x in reversed(pos)] + [0.0] + pos, dtype=np.float64)


LIMITS = _limits()


def _sum(v):
    return math.fsum(v.tolist()) if v.size <= 100000 else float(np.sum(v))


def reference(x):
    """x: float32 array (any shape) -> dict of the record's fields, over the finite values alone"""
    x = np.asarray(x, dtype=np.float32).ravel()
    fin = np.isfinite(x)
    d = x[fin].astype(np.float64)
    counts = np.bincount(np.searchsorted(LIMITS, d, side="right"), minlength=LIMITS.size).astype(np.uint32)
    return dict(counts=counts, num=float(d.size), min=float(d.min()) if d.size else np.inf, max=float(d.max()) if d.size else -np.inf,
                sum=_sum(d), sum_squares=_sum(d * d), nonfinite=float((~fin).sum()),
                abs_sum=_sum(np.abs(d)), abs_sq=_sum(d * d), n=int(d.size))


def check(got, ref, what):
    print("%-28s n %8d  sum %+.17g (ref %+.17g, bound %.3g)  sq %.17g (ref %.17g, bound %.3g)  nonfinite %d" % (
        what, ref["n"], got["sum"], ref["sum"], ref["n"] * 2.0 ** -53 * ref["abs_sum"], got["sum_squares"], ref["sum_squares"],
        ref["n"] * 2.0 ** -53 * ref["abs_sq"], got["nonfinite"]))
    assert np.array_equal(got["counts"], ref["counts"]), (what, np.nonzero(got["counts"] != ref["counts"])[0][:8])
    assert got["num"] == ref["num"] and got["nonfinite"] == ref["nonfinite"], what
    assert got["min"] == ref["min"] and got["max"] == ref["max"], (what, got["min"], ref["min"], got["max"], ref["max"])
    assert abs(got["sum"] - ref["sum"]) <= ref["n"] * 2.0 ** -53 * ref["abs_sum"], what
    assert abs(got["sum_squares"] - ref["sum_squares"]) <= ref["n"] * 2.0 ** -53 * ref["abs_sq"], what


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def records(H, raw, count):
    rec, nb = H.lib().air_histogram_record_bytes(), H.lib().air_histogram_num_buckets()
    raw = np.asarray(raw, dtype=np.uint8)
    out = []
    for h in range(count):
        r = raw[h * rec:(h + 1) * rec]
        f = r[:48].view(np.float64)
        assert int(r[48 + 4 * nb:].view(np.uint32)[0]) == 0                      # the padding word of the record
        out.append(dict(min=f[0], max=f[1], num=f[2], sum=f[3], sum_squares=f[4], nonfinite=f[5],
                        counts=r[48:48 + 4 * nb].view(np.uint32).copy()))
    return out


def launch(H, views, prescale=1.0, dyn=None, gnorm=None, fill=0x00):
    """views: (tensor holding the data, element offset of the base, rows, cols, ld, scale_kind).  -> (raw record bytes,
    guards intact).  Output and workspace are pre-filled with `fill` bytes and carry GUARD bytes of 0xA5 behind them."""
    lib = H.lib()
    descs = (H.HistogramDesc * len(views))(*[H.HistogramDesc(t.data_ptr() + 4 * off, r, c, ld, k) for t, off, r, c, ld, k in views])
    nout, nws = lib.air_histograms_output_bytes(descs, len(views)), lib.air_histograms_workspace_bytes(descs, len(views))
    assert nout == len(views) * lib.air_histogram_record_bytes() and nws > 0 and nws % 8 == 0
    out = torch.full((nout + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws = torch.full((nws + GUARD,), fill, dtype=torch.uint8, device="cuda")
    out[nout:] = 0xA5
    ws[nws:] = 0xA5
    a = H.Histograms(descs, len(views), prescale, H.ptr(dyn), H.ptr(gnorm), H.ptr(out), H.ptr(ws), nout, nws)
    H.check(lib.air_histograms(C.byref(a), H.stream(out.device)), "air_histograms")
    torch.cuda.synchronize()
    guards = bool((out[nout:] == 0xA5).all()) and bool((ws[nws:] == 0xA5).all())
    return out[:nout].cpu().numpy(), guards


def _ceil32(limit):
    f = np.float32(limit)
    return f if np.float64(f) >= limit else np.nextafter(f, np.float32(np.inf))


def special_values():
    vals = [0.0, -0.0, 1e-40, -1e-40, 3e38, -3e38]
    pos = LIMITS[LIMITS.size // 2 + 1:-1]                                        # the finite positive limits
    for lim in (pos[0], pos[np.argmin(np.abs(pos - 1.0))], pos[-1]):
        c = _ceil32(lim)
        for v in (np.nextafter(c, np.float32(0)), c, np.nextafter(c, np.float32(np.inf))):
            vals += [v, -v]
    return np.array(vals, dtype=np.float32)


def fill_values(n, rng):
    sp = special_values()
    third = max(1, n // 3)
    rnd = np.concatenate([rng.standard_normal(third).astype(np.float32) * np.float32(s) for s in (1e-8, 1.0, 1e6)])
    return np.concatenate([sp, rnd, rnd])[:n].astype(np.float32) if n > 3 else np.concatenate([sp[[1, 8, 4]], rnd])[:n]


def test_abi_edge_descriptors(H):
    chunk = H.lib().air_histogram_chunk()
    rng = np.random.default_rng(0)
    # (rows, cols, ld, misalignment of the base in floats)
    n2 = 2 * chunk + 5
    r2 = next((r for r in range(7, 64) if n2 % r == 0), 1)                        # 2 chunk + 5 elements as a matrix where it factors
    shapes = [(1, 1, 1, 0), (1, 3, 3, 0), (1, 63, 63, 0), (1, 64, 64, 0), (1, 65, 65, 0), (1, chunk - 1, chunk - 1, 0),
              (1, chunk, chunk, 0), (1, chunk + 1, chunk + 1, 0),
              (r2, n2 // r2, n2 // r2 + 3, 0),                                    # scalar loads, padded rows, chunks cut rows
              (5, 3, 8, 0),                                                       # the pad holds NaN
              (1, 64, 64, 1),                                                     # 4-byte, not 16-byte aligned base
              (130, 128, 132, 0),                                                 # 16-byte loads, padded rows, two chunks
              (7, 8, 12, 4),                                                      # 16-byte loads on a base 16 bytes into a line
              (3, 1000, 1000, 0), (3, 999, 1001, 0)]                              # normals alone: +-3e38 do not drown the sums' bound
    host, views, expect, off = [], [], [], 0
    for rows, cols, ld, mis in shapes:
        off = (off + 3) // 4 * 4 + mis
        block = np.full(rows * ld, np.nan, dtype=np.float32)
        vals = fill_values(rows * cols, rng) if rows * cols < 2900 or rows * cols > 3100 else rng.standard_normal(rows * cols).astype(np.float32)
        block.reshape(rows, ld)[:, :cols] = vals.reshape(rows, cols)
        host.append((off, block))
        views.append((off, rows, cols, ld))
        expect.append(reference(vals))
        off += rows * ld
    flat = np.full(off + 8, np.nan, dtype=np.float32)
    for o, block in host:
        flat[o:o + block.size] = block
    dev = torch.tensor(flat, device="cuda")
    v = [(dev, o, r, c, ld, 0) for o, r, c, ld in views]
    raw, guards = launch(H, v)
    assert guards
    for (o, r, c, ld), got, ref in zip(views, records(H, raw, len(v)), expect):
        check(got, ref, "view %dx%d ld %d @%d" % (r, c, ld, o))
    # the special values really sit on both sides of a limit
    sp = reference(special_values())
    # +-0.0, 1e-40 and the fp32 just below the first limit | -1e-40 and the negative of that fp32
    assert sp["counts"][LIMITS.size // 2 + 1] == 4 and sp["counts"][LIMITS.size // 2] == 2
    assert sp["counts"][-1] == 3 and sp["counts"][1] == 3 and sp["counts"][0] == 0                # DBL_MAX buckets
    # a second launch into buffers full of 0xFF bytes: the same bits
    raw2, guards2 = launch(H, v, fill=0xFF)
    assert guards2 and np.array_equal(raw, raw2)


def test_nonfinite_values_are_counted_apart(H):
    from air.summaries import decode_histograms
    rng = np.random.default_rng(1)
    x = rng.standard_normal(1000).astype(np.float32)
    x[[7, 500, 999]] = [np.nan, np.inf, -np.inf]
    clean = rng.standard_normal(10).astype(np.float32)
    dev, dev2 = torch.tensor(x, device="cuda"), torch.tensor(clean, device="cuda")
    raw, guards = launch(H, [(dev2, 0, 1, 10, 10, 0), (dev, 0, 1, 1000, 1000, 0)])
    assert guards
    got = records(H, raw, 2)
    assert got[1]["nonfinite"] == 3.0
    check(got[0], reference(clean), "finite")
    check(got[1], reference(x), "with NaN, +Inf, -Inf")
    with pytest.raises(H.AirHipError, match="the/second/tag"):
        decode_histograms(raw, ["first", "the/second/tag"])
    ok = decode_histograms(raw[:raw.size // 2], ["first"])
    assert ok["first"].num == 10 and int(ok["first"].counts.sum()) == 10


@pytest.mark.parametrize("gnorm,clip", [(4.0, 1.0), (0.25, 1.0), (3.0, 0.0), (7.3, 2.5)])
def test_scale_kinds(H, gnorm, clip):
    rng = np.random.default_rng(2)
    n = 5000
    x = np.concatenate([special_values(), rng.standard_normal(n).astype(np.float32) * np.float32(3e-4)]).astype(np.float32)
    prescale = np.float32(1.0) / np.float32(3.0)
    dyn = np.zeros(H.DYN_COUNT, dtype=np.float32)
    dyn[H.DYN_CLIP_NORM] = clip
    g32, c32 = np.float32(gnorm), np.float32(clip)
    with np.errstate(divide="ignore"):
        s = c32 * np.minimum(np.float32(1) / g32, np.float32(1) / c32) if clip > 0 else np.float32(1)
    scale2 = np.float32(prescale * s)
    assert scale2.dtype == np.float32
    dev = torch.tensor(x, device="cuda")
    raw, guards = launch(H, [(dev, 0, 1, x.size, x.size, 0), (dev, 0, 1, x.size, x.size, 1), (dev, 0, 1, x.size, x.size, 2)],
                         prescale=float(prescale), dyn=torch.tensor(dyn, device="cuda"),
                         gnorm=torch.tensor([gnorm], dtype=torch.float32, device="cuda"))
    assert guards
    got = records(H, raw, 3)
    with np.errstate(over="ignore"):
        check(got[0], reference(x), "stored")
        check(got[1], reference(x * prescale), "x * prescale")
        check(got[2], reference(x * scale2), "x * (prescale * s)")


# ---- model level: B = 4 at the training hyper-parameters ---------------------------------------------------------------
@pytest.fixture(scope="module")
def pair(H):
    from air import air_model as am
    from oracle import air_oracle as ao
    from oracle.synth import blob_canvases
    hp = dict(ao.TRAINING_HP)
    images, targets = blob_canvases(4, hp["canvas_size"], hp["max_digits"], seed=3)
    am.reset_default_graph()
    dev_i, dev_t = torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda")
    tr = am.AIRModel(dev_i, dev_t, cnn=False, train=True, scope="air", gemm_precision="fp32", **hp)
    tr.load_state_dict(ao.init_params(hp, 0))
    tr.set_noise(ao.make_noise(hp, 4, 1))
    tr.set_dynamic(z_pres_prior_log_odds=-2.0)
    te = am.AIRModel(dev_i, dev_t, cnn=False, train=False, reuse=True, scope="air", gemm_precision="fp32", **hp)
    tr.training(eager=True)
    te.forward()
    torch.cuda.synchronize()
    return tr, te


def _snapshot(m):
    st = m.store
    t = dict(params=st.params, grads=st.grads, m=st.m, v=st.v, istate=st.istate, gnorm=st.gnorm, dyn=m.dyn, scalars=m.scalars,
             recon=m.reconstruction, att=m.att, digits=m.rec_num_digits, loss_item=m.loss_per_item)
    return {k: v.detach().clone() for k, v in t.items()}


def _fixture_tags():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "summary_tags.json")))


def test_model_grad_summaries(H, pair):
    from air.summaries import decode_histograms, gradient_summaries, variable_order
    tr, _ = pair
    before = _snapshot(tr)
    buf = tr.grad_summaries()
    again = tr.grad_summaries(torch.full_like(buf, 0xFF))
    torch.cuda.synchronize()
    after = _snapshot(tr)
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])]
    assert torch.equal(buf, again)
    names = tr.grad_summary_names()
    tags = _fixture_tags()["gradients"]
    assert len(names) == 72 and names == tags[::3]
    hist = decode_histograms(buf.cpu(), names)
    full = gradient_summaries(hist)
    assert list(full) == tags
    # the restatement over the gradient views and the global norm, fetched to the host
    clip = np.float32(float(tr.dyn[H.DYN_CLIP_NORM]))
    gnorm = np.float32(float(tr.store.gnorm[0]))
    assert clip == np.float32(1.0) and gnorm > 0
    s = clip * np.minimum(np.float32(1) / gnorm, np.float32(1) / clip)
    order = variable_order()
    assert sorted(order) == sorted(tr.store.gradients) and len(order) == 36
    for which, factor in (("original", np.float32(1.0)), ("applied", np.float32(np.float32(1.0) * s))):
        for name in order:
            tag = "air/training/air/rnn/%s_0_grad_%s" % (name, which)
            g = tr.store.gradients[name].detach().cpu().numpy().astype(np.float32) * factor
            ref = reference(g)
            h = hist[tag]
            check(dict(h._asdict(), nonfinite=0.0), ref, tag[17:])
            n = ref["n"]
            # sqrt and the division are monotone and correctly rounded: the bound on the sums carries over, plus one rounding
            sq_lo, sq_hi = ref["sum_squares"] - n * 2.0 ** -53 * ref["abs_sq"], ref["sum_squares"] + n * 2.0 ** -53 * ref["abs_sq"]
            assert math.sqrt(max(sq_lo, 0.0)) * (1 - 2.0 ** -52) <= full[tag + "_norm"] <= math.sqrt(sq_hi) * (1 + 2.0 ** -52), tag
            assert abs(full[tag + "_avg"] - ref["sum"] / n) <= 2.0 ** -53 * ref["abs_sum"] + 2.0 ** -51 * abs(ref["sum"] / n), tag


def test_model_var_summaries(H, pair):
    from air.summaries import decode_histograms, variable_order
    tr, te = pair
    before = _snapshot(te)
    buf = te.var_summaries()
    torch.cuda.synchronize()
    after = _snapshot(te)
    assert all(torch.equal(before[k], after[k]) for k in before)
    names = te.var_summary_names()
    assert names == _fixture_tags()["variables"] and len(names) == 36
    hist = decode_histograms(buf.cpu(), names)
    for name, tag in zip(variable_order(), names):
        assert tag == "air_1/summaries/air/rnn/%s_0" % name
        check(dict(hist[tag]._asdict(), nonfinite=0.0), reference(te.store.variables[name].detach().cpu().numpy()), name)
    with pytest.raises(H.AirHipError):
        te.grad_summaries()
    assert torch.equal(tr.var_summaries(), buf)                                  # the variables are the scope's, not the model's


# ---- the driver ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("print_every,precision", [(0, "bf16"), (50, "fp32")])
def test_training_driver_tensorboard(tmp_path, print_every, precision):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import glob
    import io
    import tf_events
    res = str(tmp_path / "air_results")
    cmd = [sys.executable, "training.py", "-r", res, "-o", "1", "--iterations", "600", "--print-every", str(print_every),
           "--precision", precision, "--tensorboard"]
    p = subprocess.run(cmd, cwd=PKG, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    files = glob.glob(os.path.join(res, "summary", "events.out.tfevents.*"))
    assert len(files) == 1
    events = tf_events.read_events(files[0], verify=True)
    assert events[0]["file_version"] == "brain.Event:2" and "summary" not in events[0]
    tags = _fixture_tags()
    groups = {"numeric": {}, "variables": {}, "image": {}, "gradients": {}}
    img_tags = ["%s/image/%d" % (tags["image"][0], i) for i in range(60)]
    assert img_tags[0] == "air_1/summaries/reconstruction/image/0"
    for ev in events[1:]:
        got = [v["tag"] for v in ev["summary"]]
        key = {tuple(tags["numeric"]): "numeric", tuple(tags["variables"]): "variables", tuple(img_tags): "image",
               tuple(tags["gradients"]): "gradients"}[tuple(got)]
        assert ev["step"] not in groups[key]
        groups[key][ev["step"]] = ev["summary"]
    gsteps = 50 if print_every == 0 else 1
    assert sorted(groups["numeric"]) == list(range(0, 600, 50))
    assert sorted(groups["variables"]) == [0, 250, 500]
    assert sorted(groups["image"]) == [0, 500]
    assert sorted(groups["gradients"]) == [k + gsteps for k in range(0, 600, 100)]
    # the scalars are the rows of scalars.jsonl (rounded there to 5 decimals; float32 here)
    rows = {r["step"]: r for r in (json.loads(l) for l in open(os.path.join(res, "summary", "scalars.jsonl")))}
    for step, vals in groups["numeric"].items():
        for v in vals:
            want = rows[step][v["tag"][len("air_1/summaries/"):]]
            if want is None:
                assert v["simple_value"] != v["simple_value"]
            else:
                assert abs(v["simple_value"] - want) <= 0.5e-5 + 2.0 ** -23 * abs(want), (step, v["tag"])
    for vals in groups["variables"].values():
        assert all(h["histo"]["num"] > 0 and sum(h["histo"]["bucket"]) == h["histo"]["num"] for h in vals)
        assert vals[0]["histo"]["num"] == 2756 * 1024
    for vals in groups["gradients"].values():
        assert all(("histo" in v) == (i % 3 == 0) and ("simple_value" in v) == (i % 3 != 0) for i, v in enumerate(vals))
        assert all(math.isfinite(v["simple_value"]) for v in vals if "simple_value" in v)
    Image = pytest.importorskip("PIL.Image")
    for vals in groups["image"].values():
        for v in vals:
            im = v["image"]
            assert (im["height"], im["width"], im["colorspace"]) == (100, 204, 3)
            px = np.asarray(Image.open(io.BytesIO(im["encoded_image_string"])))
            assert px.shape == (100, 204, 3) and px.dtype == np.uint8 and (px[:, 100:104] == 255).all()
    if print_every == 0:
        # without the flag: no event file
        res2 = str(tmp_path / "plain")
        p2 = subprocess.run([sys.executable, "training.py", "-r", res2, "--iterations", "50", "--print-every", "0",
                             "--precision", precision], cwd=PKG, capture_output=True, text=True, timeout=900)
        assert p2.returncode == 0, p2.stderr[-2000:]
        assert os.listdir(os.path.join(res2, "summary")) == ["scalars.jsonl"]
