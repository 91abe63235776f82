"""Time of one air.vae forward + backward at the model's shapes (M = 192 rows = 64 images x 3 steps, 784 -> 512 -> 256 -> 50
-> 256 -> 512 -> 784, likelihood_std 0.3, gradients to every variable and to the inputs), per GEMM precision:

  python tools/bench_vae.py [--rows 192] [--windows 30] [--iters 50] [--out FILE]

One figure per precision: the time of an EAGER forward + backward as a user's torch code makes it (~25 launches through
ctypes and the autograd engine, so it is host-bound), as the median over `windows` timed windows of `iters` iterations
with the min / max of the windows beside it (device events around the window, after a warm-up of every shape).
It also lists the launches of the train step that do the same work inside AIRModel (bf16, B = 64), by kernel name, so that
the figures can be set beside a kernel-trace summary of the step (profiles/*_kernel_stats.txt).  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tf-attend-infer-repeat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = dict(input_dim=784, rec=(512, 256), Z=50, gen=(256, 512))


def _windows(fn, windows, iters):
    """us per iteration of `windows` windows of `iters` calls each"""
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / iters)
    return out


def _stats(v):
    return {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def bench(prec, M, windows, iters):
    from air.vae import VAE
    m = VAE(SIZES["input_dim"], SIZES["rec"], SIZES["Z"], SIZES["gen"], likelihood_std=0.3, precision=prec)
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    x = torch.rand(M, SIZES["input_dim"], device="cuda", generator=g).requires_grad_(True)
    eps_z, eps_x = rnd(M, SIZES["Z"]), rnd(M, SIZES["input_dim"])
    d_rec, d_mean, d_lv = rnd(M, SIZES["input_dim"]), rnd(M, SIZES["Z"]), rnd(M, SIZES["Z"])
    leaves = [x] + list(m.parameters())

    def step():
        for t in leaves:
            t.grad = None
        rec, mean, lv, _ = m(x, eps_z=eps_z, eps_x=eps_x)
        torch.autograd.backward((rec, mean, lv), (d_rec, d_mean, d_lv))

    for _ in range(5):
        step()
    torch.cuda.synchronize()
    return {"eager": _stats(_windows(step, windows, iters))}


def model_launches(B=64):
    """(tag, kernel) of the train step's launches that cover the VAE, forward and backward (bf16 path)"""
    from air import air_model as am
    am.reset_default_graph()
    model = am.AIRModel(torch.zeros(B, 2500, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"), cnn=False,
                        train=True, gemm_precision="bf16", scope="bench_vae")
    tags = ("vae_", "ml_reparam", "dgrad_gen", "dz_reparam", "dgrad_rec", "dgrad_win", "wgrad_grouped")
    ops = [(op.name, op.kernel) for op in model.train_step_ops() if op.name.startswith(tags)]
    am.reset_default_graph()
    return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=192)
    ap.add_argument("--windows", type=int, default=30)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_vae.py needs the GPU: a CPU run gives no time")
    res = {"rows": a.rows, "sizes": SIZES, "windows": a.windows, "iters": a.iters}
    for prec in ("bf16", "fp32"):
        res[prec] = bench(prec, a.rows, a.windows, a.iters)
    res["model_launches_bf16"] = model_launches()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
