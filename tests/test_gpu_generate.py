"""Generation on the device: AIRModel.generate() (scenes from the priors), AIRModel.decode() (scenes from the caller's
latents), the render kernel behind both, their Philox stream, and the wrapper / demo around them.

The reference of the parity test is a numpy restatement of the generative half of the loop body (air_model.py:288-439, 582;
vae.py:26-41) with the posterior heads replaced by the priors, built from the oracle's helpers.  Bands: the project's own
(tests/test_gpu_model.py): canvas 2e-5 (fp32) / 3e-2 (bf16), per-step quantities 5e-5 * max(1, |ref|), counts exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import air_oracle as ao
from oracle.synth import blob_canvases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tf-attend-infer-repeat_amd")
HP = dict(ao.TRAINING_HP)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def am():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model
    return air_model


def _np(t):
    return t.detach().cpu().numpy()


def _model(am, B, train=False, prec="fp32", scope="air", hp=HP, seed=0, images=None, reset=True, **kw):
    if reset:
        am.reset_default_graph()
    C2 = hp["canvas_size"] ** 2
    img = torch.zeros(B, C2, device="cuda") if images is None else torch.tensor(images, device="cuda")
    m = am.AIRModel(img, torch.zeros(B, dtype=torch.int32, device="cuda"), cnn=False, train=train, scope=scope,
                    gemm_precision=prec, seed=seed, **kw, **hp)
    return m


def reference_generate(params, noise, hp, prior_log_odds, likelihood_noise):
    """The semantics of AIRModel.generate() in numpy fp32, step by step."""
    f = np.float32
    N, Cc, w = hp["max_steps"], hp["canvas_size"], hp["windows_size"]
    B = noise["u"].shape[1]
    thr, temp = f(hp["stopping_threshold"]), hp["z_pres_temperature"]
    sigma = f(hp["vae_likelihood_std"] if likelihood_noise else 0.0)
    S = np.zeros(B, f)
    R = np.zeros((B, Cc * Cc), f)
    digits = np.zeros(B, np.int32)
    out = {k: [] for k in ("scales", "shifts", "z_pres", "masks", "latents", "windows", "st_back")}
    for t in range(N):
        scale = ao.sigmoid(f(hp["scale_prior_mean"]) + np.sqrt(f(hp["scale_prior_variance"])) * noise["eps_scale"][t])    # [B,1]
        shift = np.tanh(f(hp["shift_prior_mean"]) + np.sqrt(f(hp["shift_prior_variance"])) * noise["eps_shift"][t])     # [B,2]
        z_what = f(hp["vae_prior_mean"]) + np.sqrt(f(hp["vae_prior_variance"])) * noise["eps_z"][t]                     # [B,Z]
        z_pre = ao.concrete_binary_pre_sigmoid_sample(np.full(B, prior_log_odds, f), temp, noise["u"][t])
        z_pres = np.round(ao.sigmoid(z_pre))
        S = S + (f(1.0) - z_pres)
        mask = S < thr
        digits = digits + mask.astype(np.int32)
        h = z_what
        for i in range(len(hp["vae_generative_units"])):
            h = ao.fully_connected(h, params["vae/generative_%d/weights" % (i + 1)],
                                   params["vae/generative_%d/biases" % (i + 1)], "softplus")
        gen_mean = ao.fully_connected(h, params["vae/gen_mean/weights"], params["vae/gen_mean/biases"])
        window = ao.sigmoid(gen_mean + noise["eps_x"][t] * sigma)
        s, x, y = scale[:, 0], shift[:, 0], shift[:, 1]
        zeros = np.zeros_like(s)
        theta = np.stack([np.stack([f(1.0) / s, zeros, -x / s], axis=1), np.stack([zeros, f(1.0) / s, -y / s], axis=1)], axis=1)
        wr = ao.transformer(window.reshape(B, w, w), theta, (Cc, Cc)).reshape(B, Cc * Cc)
        R = R + np.where(mask[:, None], z_pres[:, None] * wr, np.zeros_like(R))
        for k, v in (("scales", scale), ("shifts", shift), ("z_pres", z_pres), ("masks", mask.astype(f)), ("latents", z_what),
                     ("windows", window), ("st_back", np.stack([f(1.0) / s, -x / s, -y / s], axis=1))):
            out[k].append(v)
    res = {k: np.swapaxes(np.stack(v), 0, 1) for k, v in out.items()}          # image-major
    res["canvas"] = np.maximum(np.minimum(R, f(1.0)), f(0.0))
    res["num_digits"] = digits
    return res


@pytest.mark.parametrize("likelihood_noise", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_generate_parity_with_injected_noise(am, prec, likelihood_noise):
    B = 64
    noise = ao.make_noise(HP, B, seed=2)
    gap = float(np.abs(noise["u"] - 0.5).min())
    print("min |u - 0.5| = %.3e" % gap)
    assert gap >= 5e-4                                       # no rounding tie of z_pres is near
    params = ao.init_params(HP, 0)
    model = _model(am, B, prec=prec)
    model.load_state_dict(params)
    model.set_dynamic(z_pres_prior_log_odds=0.0)
    model.set_generate_noise(noise)
    sc = model.generate(likelihood_noise=likelihood_noise)
    torch.cuda.synchronize()
    ref = reference_generate(params, noise, HP, 0.0, likelihood_noise)
    hist = np.bincount(ref["num_digits"], minlength=4).tolist()
    print("scenes with 0 / 1 / 2 / 3 objects:", hist)
    assert all(h > 0 for h in hist)                           # every class and the mask logic are exercised
    d_canvas = float(np.abs(_np(sc.canvas) - ref["canvas"]).max())
    print("%s likelihood_noise=%s: |d canvas| = %.3e" % (prec, likelihood_noise, d_canvas))
    assert np.array_equal(_np(sc.num_digits), ref["num_digits"])
    assert np.array_equal(_np(sc.z_pres), ref["z_pres"])
    assert np.array_equal(_np(sc.masks), ref["masks"])
    for k in ("scales", "shifts", "latents", "st_back"):      # no GEMM in front of them: the fp32 band in both precisions
        got = _np(getattr(sc, k))
        assert got.shape == ref[k].shape, (k, got.shape, ref[k].shape)
        d = float(np.abs(got - ref[k]).max())
        print("  |d %s| = %.3e" % (k, d))
        assert d <= 5e-5 * max(1.0, float(np.abs(ref[k]).max())), (k, d)
    d_win = float(np.abs(_np(sc.windows) - ref["windows"]).max())
    print("  |d windows| = %.3e" % d_win)
    if prec == "fp32":
        assert d_canvas <= 2e-5
        assert d_win <= 5e-5
    else:
        assert d_canvas <= 3e-2


def _forward_model(am, B, train, prec, scope, seed_noise=1, reset=True):
    images, _ = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=3)
    noise = ao.make_noise(HP, B, seed_noise)
    model = _model(am, B, train=train, prec=prec, scope=scope, images=images, reset=reset)
    model.load_state_dict(ao.init_params(HP, 0))
    model.set_noise(noise)
    model.set_dynamic(z_pres_prior_log_odds=-2.0)
    return model, noise


def _decode_own_pass(model, noise):
    H = sys.modules["air._hip"]
    att = model.att
    model.set_generate_noise(noise)
    return model.decode(model.zs.transpose(0, 1), att[:, :, H.ATT_S:H.ATT_S + 1].transpose(0, 1),
                        att[:, :, H.ATT_X:H.ATT_Y + 1].transpose(0, 1), att[:, :, H.ATT_Z].t(), likelihood_noise=True)


@pytest.mark.parametrize("train", [False, True])
def test_decode_reproduces_the_forward_fp32(am, train):
    model, noise = _forward_model(am, 64, train, "fp32", "air")
    model.forward()
    torch.cuda.synchronize()
    keep = {k: getattr(model, k).clone() for k in ("reconstruction", "loss", "normals", "uniforms", "att", "vrec", "rec_num_digits")}
    step, dyn = int(model.global_step), model.dyn.clone()
    sc = _decode_own_pass(model, noise)
    torch.cuda.synchronize()
    T = model.steps_executed
    assert torch.equal(sc.canvas, model.reconstruction)
    assert torch.equal(sc.windows[:, :T], model.rec_windows)
    assert torch.equal(sc.num_digits, model.rec_num_digits)
    # the decode call left the pass alone
    for k, v in keep.items():
        assert torch.equal(getattr(model, k), v), k
    assert int(model.global_step) == step and torch.equal(model.dyn, dyn)


@pytest.mark.parametrize("train", [False, True])
def test_decode_bf16_against_fp32_decode(am, train):
    mb, noise = _forward_model(am, 64, train, "bf16", "air")
    mb.forward()
    torch.cuda.synchronize()
    keep = {k: getattr(mb, k).clone() for k in ("reconstruction", "loss", "normals", "uniforms")}
    sb = _decode_own_pass(mb, noise)
    H = sys.modules["air._hip"]
    mf = _model(am, 64, train=False, prec="fp32", scope="f32", reset=False)
    mf.load_state_dict(ao.init_params(HP, 0))
    mf.set_generate_noise(noise)
    sf = mf.decode(sb.latents.contiguous(), sb.scales.contiguous(), sb.shifts.contiguous(), sb.z_pres.contiguous(),
                   likelihood_noise=True)
    torch.cuda.synchronize()
    d = float((sb.canvas - sf.canvas).abs().max())
    print("train=%s: |canvas bf16 decode - fp32 decode| = %.3e, against the bf16 forward %.3e"
          % (train, d, float((sb.canvas - mb.reconstruction).abs().max())))
    assert d <= 3e-2
    assert torch.equal(sb.num_digits, sf.num_digits) and torch.equal(sb.num_digits, mb.rec_num_digits)
    for k, v in keep.items():
        assert torch.equal(getattr(mb, k), v), k
    assert H.ATT_STRIDE == 16


def _scene_records_given(H, scales, shifts, latents, z_pres, dyn):
    """air_scene_records(given = 1): att [N,B,16] from the caller's scales [N,B], shifts [N,B,2], latents [N,B,Z], z_pres [N,B]"""
    N, B, Z = latents.shape
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    att = torch.full((N, B, H.ATT_STRIDE), float("nan"), device="cuda")
    z = torch.full((N, B, Z), float("nan"), device="cuda")
    a = H.SceneRecords(p(scales), p(shifts), p(latents), p(z_pres), p(dyn), p(att), p(z), None, B, N, Z, Z, 1)
    H.check(H.lib().air_scene_records(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "air_scene_records")
    return att


@pytest.mark.parametrize("Cc,N", [pytest.param(50, 5, id="50"), pytest.param(128, 5, id="128"),
                                  pytest.param(50, 16, id="50-16-steps-given-records")])
def test_render_equals_compose_bit_for_bit(am, Cc, N):
    H = sys.modules["air._hip"]
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    if N == 16:
        # all 16 steps the records of the two kernels hold, without a model: records from air_scene_records on scales,
        # shifts and (relaxed) z_pres given by the caller -- image 0 alive through all 16 steps, 1 stops at step 0, 2 at
        # step 7, 3 at step 15 -- and random windows; air_write_fwd and air_render on the same att / vrec
        B, w, Z = 4, 28, 3
        rng = np.random.RandomState(16)
        z_pres = rng.uniform(0.97, 0.999, (N, B)).astype(np.float32)
        z_pres[0, 1] = z_pres[7, 2] = z_pres[15, 3] = 0.004
        t_ = lambda a: torch.tensor(a.astype(np.float32), device="cuda")  # noqa: E731
        dyn = np.zeros(H.DYN_COUNT, np.float32)
        dyn[H.DYN_STOP_THRESHOLD], dyn[H.DYN_GRAD_SCALE], dyn[H.DYN_VAE_PV] = 0.99, 1.0 / B, 1.0
        dyn_d = t_(dyn)
        att = _scene_records_given(H, t_(rng.uniform(0.2, 0.95, (N, B))), t_(rng.uniform(-0.8, 0.8, (N, B, 2))),
                                   t_(rng.standard_normal((N, B, Z))), t_(z_pres), dyn_d)
        vrec = t_(rng.uniform(0.0, 0.4, (N, B, w * w)))
        images, _ = blob_canvases(B, Cc, 2, seed=3)
        recon, rec_loss, run_loss, loss_item = (torch.full(s, float("nan"), device="cuda") for s in ((B, Cc * Cc), (B,), (B,), (B,)))
        run_digits = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        ml, img_d = torch.zeros(N, B, 2 * Z, device="cuda"), torch.tensor(images, device="cuda")
        att_w = att.clone()
        wf = H.WriteFwd(p(vrec), p(ml), p(img_d), p(dyn_d), p(att_w), p(recon), p(rec_loss), None, p(run_loss), p(run_digits),
                        p(loss_item), B, N, Cc, w, Z, None)
        H.check(H.lib().air_write_fwd(C.byref(wf), stream()), "air_write_fwd")
        canvas = torch.full((B, Cc * Cc), -1.0, device="cuda")
        digits = torch.full((B,), -1, dtype=torch.int32, device="cuda")
        a = H.Render(p(vrec), p(att), p(canvas), p(digits), B, N, Cc, w)
        H.check(H.lib().air_render(C.byref(a), stream()), "air_render")
        torch.cuda.synchronize()
        assert digits.tolist() == [16, 0, 7, 15]                  # the stopping sum of air_scene_records, in step order
        assert torch.equal(att[:, :, H.ATT_MASK].sum(0).to(torch.int32), digits)
        assert torch.equal(digits, run_digits)
        assert torch.equal(canvas, recon)
        assert float(canvas[0].max()) == 1.0 and not bool(canvas[1].any()) and float(canvas.min()) == 0.0
        return
    hp = dict(HP, canvas_size=Cc, max_steps=5)
    B, w = 16, hp["windows_size"]
    images, _ = blob_canvases(B, Cc, hp["max_digits"], seed=3)
    model = _model(am, B, hp=hp, images=images)
    model.load_state_dict(ao.init_params(hp, 0))
    noise = ao.make_noise(hp, B, 1)
    noise["u"] = (0.5 + 0.5 * noise["u"]).astype(np.float32)  # Concrete noise >= 0: most steps active, several windows per pixel
    model.set_noise(noise)
    model.forward()
    torch.cuda.synchronize()
    canvas = torch.full((B, Cc * Cc), -1.0, device="cuda")
    digits = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    a = H.Render(p(model.vrec), p(model.att), p(canvas), p(digits), B, N, Cc, w)
    H.check(H.lib().air_render(C.byref(a), stream()), "air_render")
    torch.cuda.synchronize()
    print("C = %d: active (image, step) pairs %d of %d" % (Cc, int(model.rec_num_digits.sum()), B * N))
    assert int(model.rec_num_digits.max()) >= 2              # overlapping windows: the step-order sum is exercised
    assert torch.equal(canvas, model.reconstruction)
    assert torch.equal(digits, model.rec_num_digits)


def _within(frac, p, n, what):
    sd = np.sqrt(p * (1.0 - p) / n)
    print("  %s: %.4f, expected %.4f +- 4.5 x %.4f" % (what, frac, p, sd))
    assert abs(frac - p) <= 4.5 * sd, (what, frac, p, sd)


def test_device_rng_statistics_reproducibility_and_non_interference(am):
    B, calls = 512, 8
    model = _model(am, B, scope="a", seed=11)
    model.set_dynamic(z_pres_prior_log_odds=0.0)
    step, dyn = int(model.global_step), model.dyn.clone()
    counts, scales, shifts, first = [], [], [], []
    for c in range(calls):
        sc = model.generate()
        counts.append(_np(sc.num_digits).copy()); scales.append(_np(sc.scales).copy()); shifts.append(_np(sc.shifts).copy())
        if c < 2:
            first.append({k: getattr(sc, k).clone() for k in ("canvas", "latents", "scales", "shifts", "z_pres", "windows")})
    torch.cuda.synchronize()
    assert int(model.global_step) == step and torch.equal(model.dyn, dyn)          # non-interference
    counts = np.concatenate(counts)
    n = counts.size
    assert n == 4096
    # P(z_pres = 1) = sigmoid(log-odds) = 1/2 for any temperature; the stopping rule ends a scene at its first 0
    for k, p in enumerate((0.5, 0.25, 0.125, 0.125)):
        _within(float(np.mean(counts == k)), p, n, "%d objects" % k)
    f = np.float64
    pm, sd = f(HP["scale_prior_mean"]), np.sqrt(f(HP["scale_prior_variance"]))
    s = np.concatenate(scales).astype(f).ravel()
    logit = np.log(s) - np.log1p(-s)
    _within(float(np.mean(logit < pm)), 0.5, s.size, "logit(scale) below the prior mean")
    _within(float(np.mean(np.abs(logit - pm) < sd)), 0.6827, s.size, "logit(scale) within one prior sd")
    pm, sd = f(HP["shift_prior_mean"]), np.sqrt(f(HP["shift_prior_variance"]))
    h = np.concatenate(shifts).astype(f).ravel()
    _within(float(np.mean(h < np.tanh(pm))), 0.5, h.size, "shift below tanh(prior mean)")
    _within(float(np.mean((h > np.tanh(pm - sd)) & (h < np.tanh(pm + sd)))), 0.6827, h.size, "shift within tanh(mean +- sd)")
    # distinctness: successive calls draw different scenes
    assert not torch.equal(first[0]["latents"], first[1]["latents"])
    assert not torch.equal(first[0]["canvas"], first[1]["canvas"])
    # reproducibility: a second model with the same seed agrees bit for bit, call by call
    twin = _model(am, B, scope="b", seed=11, reset=False)
    twin.set_dynamic(z_pres_prior_log_odds=0.0)
    for c in range(2):
        sc = twin.generate()
        for k, v in first[c].items():
            assert torch.equal(getattr(sc, k), v), (c, k)
    # ... and another seed does not
    other = _model(am, B, scope="c", seed=12, reset=False)
    assert not torch.equal(other.generate().latents, first[0]["latents"])


def test_wrapper_generate_and_demo(am, tmp_path):
    from demo.model_wrapper import ModelWrapper
    model = _model(am, 64)
    model.load_state_dict(ao.init_params(HP, 0))
    model.set_dynamic(z_pres_prior_log_odds=0.0)
    counts, positions, canvases, windows, latents = ModelWrapper(model, None, None).generate(70)
    assert len(counts) == len(positions) == len(canvases) == len(windows) == len(latents) == 70
    assert 0 < sum(counts) < 70 * HP["max_steps"]
    for i in range(70):
        assert len(positions[i]) == counts[i] and len(windows[i]) == counts[i] and len(latents[i]) == counts[i]
        assert canvases[i].shape == (50, 50)
        if counts[i]:
            assert positions[i].shape == (counts[i], 3) and windows[i].shape == (counts[i], 28, 28)
    assert not np.array_equal(np.stack(canvases[:6]), np.stack(canvases[64:]))      # the second batch is another draw
    ckpt = str(tmp_path / "air-model.pt")
    torch.save(model.state_dict(), ckpt)
    out = str(tmp_path / "out")
    p = subprocess.run([sys.executable, "demo.py", "--model", ckpt, "--generate", "16", "--prior-log-odds", "0.0", "--out", out],
                       cwd=PKG, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    png = os.path.join(out, "generated_samples.png")
    assert os.path.getsize(png) > 1000
    from PIL import Image
    with Image.open(png) as im:
        assert im.size[0] > 8 * 204 and im.size[1] > 2 * 100
    rows = json.load(open(os.path.join(out, "generated.json")))
    assert len(rows) == 16 and all(len(r["positions_s_x_y"]) == r["objects"] for r in rows)


def test_generation_survives_a_rebuild_of_the_programs(am):
    """Host-side state only: a rebuild of the model's programs (set_backward, use_device_rng(seed)) drops the generation
    launch lists and keeps the generation buffers -- no stale launch list, no reallocated buffer.  Independent of shape, so
    the smallest model the kernels take; everything is compared bit for bit."""
    B, N, Z, w = 3, 2, 6, 8
    am.reset_default_graph()
    model = am.AIRModel(torch.zeros(B, 16 * 16, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), cnn=False,
                        train=True, scope="rebuild", gemm_precision="bf16", max_steps=N, canvas_size=16, windows_size=w,
                        rnn_units=32, vae_latent_dimensions=Z, vae_recognition_units=(16,), vae_generative_units=(16,),
                        scale_hidden_units=8, shift_hidden_units=8, z_pres_hidden_units=8)
    model.set_dynamic(z_pres_prior_log_odds=4.0)
    rng = np.random.RandomState(3)
    noise = {"eps_scale": rng.randn(N, B, 1), "eps_shift": rng.randn(N, B, 2), "eps_z": rng.randn(N, B, Z),
             "eps_x": rng.randn(N, B, w * w),
             # z_pres = 1 where log-odds + logit(u) > 0: every step but the last scene's second one
             "u": np.array([[0.5, 0.6, 0.7], [0.4, 0.3, 0.01]])}
    fields = am.GeneratedScenes.__slots__
    assert len(fields) == 9

    model.set_generate_noise(noise)
    sc = model.generate()
    first = {k: getattr(sc, k).clone() for k in fields}
    ptrs = {k: getattr(sc, k).data_ptr() for k in fields}
    assert first["num_digits"].tolist() == [2, 2, 1] and float(first["canvas"].abs().sum()) > 0

    def decoded_canvas():
        return model.decode(first["latents"], first["scales"], first["shifts"], first["z_pres"]).canvas

    assert torch.equal(decoded_canvas(), first["canvas"])
    model.set_backward("exact")                              # rebuilds the programs
    model.set_generate_noise(noise)
    sc = model.generate()
    for k in fields:
        assert torch.equal(getattr(sc, k), first[k]), k
        assert getattr(sc, k).data_ptr() == ptrs[k], k
    assert torch.equal(decoded_canvas(), first["canvas"])
    model.use_device_rng(seed=7)                             # ... and again
    assert torch.equal(decoded_canvas(), first["canvas"])
    torch.cuda.synchronize()
