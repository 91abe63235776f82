"""Times the captured train step of AIRModel(cnn=True) beside the same step with cnn=False, from one process: the defaults
of the constructor (S = 50, F = 8, three steps) at B = 64, bf16 and fp32, device RNG, 100 train steps per replay.  Every
model is warmed up by two replays; then three rounds alternate the four models, each round timing five replays between two
device events.  Prints the median over the rounds, the spread, the launch count of a step and one JSON line.  Nothing is
asserted: these are numbers for the record.

    python tools/bench_cnn_step.py [B [steps per replay]]
    python tools/bench_cnn_step.py --trace PREC      one eager cnn=True step loop for `rocprofv3 --kernel-trace --stats -- ...`
                                                      (per-launch times of cnn_fwd_kernel, the dgrad GEMM, cnn_bwd_kernel,
                                                      cnn_reduce_sq_kernel: tools/rocprof_summary.py reads the csv)"""
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
    sys.exit("bench_cnn_step needs the GPU: there is nothing to time without one")
trace = sys.argv[1] == "--trace" if len(sys.argv) > 1 else False
args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = 64 if trace or not args else int(args[0])
G = 100 if trace or len(args) < 2 else int(args[1])
images, targets = blob_canvases(B, 50, 2, seed=7)
x, t = torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda")


def model(prec, cnn):
    return am.AIRModel(x, t, cnn=cnn, train=True, scope="%s_%d" % (prec, cnn), gemm_precision=prec,
                       backward=am.TRAINING_BACKWARD, learning_rate=1e-4, gradient_clipping_norm=1.0)


if trace:
    m = model(args[0] if args else "bf16", True)
    for _ in range(60):
        m.training(eager=True)
    torch.cuda.synchronize()
    print("traced 60 eager cnn=True steps (%s), loss %.3f" % (m.gemm_precision, float(m.loss)))
    sys.exit(0)

models = {(prec, cnn): model(prec, cnn) for prec in ("bf16", "fp32") for cnn in (False, True)}
for m in models.values():
    m.capture_graph(steps=G)
    m.training()
    m.training()
torch.cuda.synchronize()


def timeit(m, replays=5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        m.training()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (replays * G) * 1e3


res = {k: [] for k in models}
for _ in range(3):
    for k, m in models.items():
        res[k].append(timeit(m))
out = {}
for (prec, cnn), v in res.items():
    key = "%s_cnn%d" % (prec, cnn)
    out[key] = dict(us_per_step=sorted(v)[1], spread=(max(v) - min(v)) / sorted(v)[1], launches=len(models[(prec, cnn)].train_step_ops()),
                    final_loss=float(models[(prec, cnn)].loss))
    print("%s cnn=%s: %.1f us per captured step (median of 3 rounds of %d steps, spread %.1f %%), %d launches per step, loss %.2f"
          % (prec, cnn, out[key]["us_per_step"], 5 * G, 100 * out[key]["spread"], out[key]["launches"], out[key]["final_loss"]), flush=True)
print(json.dumps({"B": B, "steps_per_replay": G, "results": out}))
