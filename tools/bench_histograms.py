"""Times the two histogram-summary launches of the model at the default shapes (AIRModel.var_summaries: 36 histograms of the
variables; grad_summaries: 72 of the gradients, original and applied -- one air_histograms call each) against the chain a
user would otherwise write in torch on the device: per tensor torch.bucketize against TensorFlow's limits + bincount + the
five reductions (min, max, numel, sum, sum of squares in float64), from contiguous copies of the views.  50 back-to-back
calls between two device events after a warm-up, three repeats alternating the versions; prints the median of the repeats,
the spread and one JSON line.
    python tools/bench_histograms.py [fp32|bf16]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch
from bench import HP, ANNEAL, synthetic_canvases
from air import air_model as am, _hip as H
from air.summaries import histogram_limits, variable_order

prec = sys.argv[1] if len(sys.argv) > 1 else "bf16"
hp, B = dict(HP), 64
images, targets = synthetic_canvases(B, hp["canvas_size"], hp["max_digits"], 1)
m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=True,
                annealing_schedules=ANNEAL, gemm_precision=prec, **hp)
for _ in range(3):
    m.training()
torch.cuda.synchronize()
limits = torch.tensor(histogram_limits(), device="cuda")
order = variable_order(len(m.vae_recognition_units), len(m.vae_generative_units))
var_out, grad_out = m.var_summaries(), m.grad_summaries()


def timeit(fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


def torch_one(t):
    d = t.reshape(-1).double()
    idx = torch.bucketize(d, limits, right=True)
    return torch.bincount(idx, minlength=limits.numel()), d.min(), d.max(), d.numel(), d.sum(), (d * d).sum()


def torch_vars():
    return [torch_one(m.store.variables[k]) for k in order]


def torch_grads():
    clip, g = m.dyn[H.DYN_CLIP_NORM], m.store.gnorm[0]
    s = clip * torch.minimum(1.0 / g, 1.0 / clip)
    return [torch_one(m.store.gradients[k]) for k in order] + [torch_one(m.store.gradients[k] * s) for k in order]


# the two chains agree on the counts (the fused launch is exact: tests/test_gpu_histograms.py)
nb, rec = limits.numel(), H.lib().air_histogram_record_bytes()
counts = var_out.cpu().numpy().reshape(len(order), rec)[:, 48:48 + 4 * nb].copy().view("uint32")
ref = torch.stack([r[0] for r in torch_vars()]).cpu().numpy()
assert (counts == ref).all()

runs = (("hip_var_summaries", lambda: m.var_summaries(var_out)), ("torch_var_chain", torch_vars),
        ("hip_grad_summaries", lambda: m.grad_summaries(grad_out)), ("torch_grad_chain", torch_grads))
res = {k: [] for k, _ in runs}
for _ in range(3):
    for k, fn in runs:
        res[k].append(timeit(fn))
med = {k: sorted(v)[1] for k, v in res.items()}
spread = {k: (max(v) - min(v)) / sorted(v)[1] for k, v in res.items()}
n_el = sum(v.numel() for v in m.store.variables.values())
print("%d elements in 36 variables: var_summaries %.1f us fused, %.1f us torch chain; grad_summaries (72 histograms) %.1f us "
      "fused, %.1f us torch chain; largest spread over 3 repeats %.0f%%" %
      (n_el, med["hip_var_summaries"], med["torch_var_chain"], med["hip_grad_summaries"], med["torch_grad_chain"],
       100 * max(spread.values())), flush=True)
print(json.dumps({"precision": prec, "elements": n_el, "median_us": med, "spread": spread}))
