"""Times the captured train step of AIRModel(likelihood="gaussian") beside two Bernoulli models of the same build, from one
process: compose_fold=False (the same launch count: the fold is not taught the Gaussian likelihood, so this is the
like-for-like arm) and the default (compose inside the write-backward launch: what the missing fold costs).  bench.py's
flagship shapes (the constructor's defaults, B = 64, bf16, device RNG); the protocol of tools/ab.sh: 40 warm-up steps, 400
timed steps per round, here as alternating rounds in one session.  Prints the median over the rounds, the spread, the
launch count of a captured step and one JSON line.  Nothing is asserted: numbers for the record.

    python tools/bench_likelihood.py [B [rounds]]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch  # noqa: E402
from air import air_model as am  # noqa: E402
from oracle.synth import blob_canvases  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("bench_likelihood needs the GPU: there is nothing to time without one")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
G, WARMUP, STEPS = 40, 40, 400                       # steps per replay; warm-up and timed steps as tools/ab.sh
images, targets = blob_canvases(B, 50, 2, seed=7)
x, t = torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda")
ARMS = {"gaussian": dict(likelihood="gaussian"), "bernoulli_no_fold": dict(compose_fold=False), "bernoulli": dict()}


def model(name, kw):
    return am.AIRModel(x, t, cnn=False, train=True, scope=name, gemm_precision="bf16", backward=am.TRAINING_BACKWARD,
                       learning_rate=1e-4, gradient_clipping_norm=1.0, **kw)


models = {name: model(name, kw) for name, kw in ARMS.items()}
for m in models.values():
    m.capture_graph(steps=G)
    for _ in range(WARMUP // G):
        m.training()
torch.cuda.synchronize()


def timeit(m):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(STEPS // G):
        m.training()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / STEPS


res = {k: [] for k in models}
for _ in range(ROUNDS):
    for k, m in models.items():
        res[k].append(timeit(m))
out = {}
for k, v in res.items():
    med = sorted(v)[len(v) // 2]
    out[k] = dict(ms_per_step=med, spread=(max(v) - min(v)) / med, launches=len(models[k].captured_step_ops(1)),
                  final_loss=float(models[k].loss))
    print("%-18s %.4f ms per captured step (median of %d rounds of %d steps, spread %.1f %%), %d launches per step, loss %.2f"
          % (k, med, ROUNDS, STEPS, 100 * out[k]["spread"], out[k]["launches"], out[k]["final_loss"]), flush=True)
print("gaussian - bernoulli_no_fold: %+.2f us; bernoulli_no_fold - bernoulli (the fold): %+.2f us"
      % (1e3 * (out["gaussian"]["ms_per_step"] - out["bernoulli_no_fold"]["ms_per_step"]),
         1e3 * (out["bernoulli_no_fold"]["ms_per_step"] - out["bernoulli"]["ms_per_step"])))
print(json.dumps({"B": B, "steps_per_replay": G, "rounds": ROUNDS, "results": out}))
