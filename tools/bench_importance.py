"""The importance-weighted bound (air.metrics.ImportanceBound, air_importance_logw / air_importance_fold) beside the passes
it scores.

  python tools/bench_importance.py [B [K [precision]]]
      At T = 3, Z = 50 (rows of 52), B images (default 64) and K samples (default 16): 55 eager air_importance_logw calls and 55
      air_importance_fold calls on synthetic records (tests/importance_cases.py), then a test model of the training driver's
      hyper-parameters at that batch: 55 eager forward(), 55 forward_sampled() and 20 ImportanceBound.evaluate() + values().
      Prints HIP-event times; meant to run under `rocprofv3 --kernel-trace --stats` in a run of its own for the launch times
      (tools/rocprof_summary.py)."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import importance_cases as ic
from air import _hip as H
from air import air_model as am
from air.metrics import ImportanceBound
from oracle import air_oracle as ao
from oracle.synth import blob_canvases

dev = torch.device("cuda", 0)
T, Z, LDZ = 3, 50, 52


def timed(fn, n=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def main(B, K, precision):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                # noqa: E731
    inp = ic.logw_inputs((B, B, T, Z, LDZ, K))
    t = {key: up(inp[key]) for key in ("att", "out7", "ml", "z", "eps_scale", "eps_shift", "eps_z", "rec_loss", "run_digits", "dyn")}
    logw = torch.zeros(K, B, dtype=torch.float64, device=dev)
    digits = torch.zeros(K, B, dtype=torch.int32, device=dev)
    a = H.Importance(*(H.ptr(t[key]) for key in ("att", "out7", "ml", "z", "eps_scale", "eps_shift", "eps_z", "rec_loss",
                                                  "run_digits", "dyn")), H.ptr(logw), H.ptr(digits), None, T, B, B, Z, LDZ, K)
    for s in range(K):
        H.launch("air_importance_logw", dev, C.byref(a), s)
    t_logw = timed(lambda: H.launch("air_importance_logw", dev, C.byref(a), 0))
    counts = torch.zeros(ic.COUNTS + (T + 1) * (T + 1), dtype=torch.int64, device=dev)
    sums = torch.zeros(ic.SUMS, dtype=torch.float64, device=dev)
    ws = torch.empty(H.lib().air_importance_fold_workspace_bytes(T, B, B, K) // 8, dtype=torch.float64, device=dev)
    f = H.ImportanceFold(H.ptr(logw), H.ptr(digits), H.ptr(t["run_digits"]), None, None, None, H.ptr(counts), H.ptr(sums), T, B, B, K)
    t_fold = timed(lambda: H.launch("air_importance_fold", dev, C.byref(f), H.ptr(ws)))
    print("importance bound, B = %d, T = %d, Z = %d, K = %d: %.1f us per air_importance_logw (one launch), %.1f us per "
          "air_importance_fold (two launches), eager, HIP events" % (B, T, Z, K, t_logw, t_fold))

    hp = dict(ao.TRAINING_HP)
    images, targets = blob_canvases(B, hp["canvas_size"], hp["max_digits"], seed=5)
    am.reset_default_graph()
    m = am.AIRModel(torch.tensor(images, device=dev), torch.tensor(targets, device=dev), cnn=False, train=False, scope="air",
                    gemm_precision=precision, **hp)
    m.load_state_dict(ao.init_params(hp, 0))
    t_fwd = timed(m.forward)
    calls = iter(range(10 ** 6))
    t_sampled = timed(lambda: m.forward_sampled(next(calls)))
    iw = ImportanceBound(m, samples=K)
    tg = torch.tensor(np.asarray(targets, np.int32), device=dev)

    def evaluation():
        iw.evaluate(tg)
        iw.values()
    t_eval = timed(evaluation, n=20)
    res = iw.result()
    print("  %s test model at that batch: %.1f us per eager forward(), %.1f us per forward_sampled() (air_philox_fill + the "
          "forward on given noise), %.1f us per evaluate() + values() = %.2f x K forward_sampled()" %
          (precision, t_fwd, t_sampled, t_eval, t_eval / (K * t_sampled)))
    print("  last evaluation: " + "  ".join("%s %.4f" % (k, res[k]) for k in ic.NAMES))


if __name__ == "__main__":
    argv = sys.argv[1:]
    main(int(argv[0]) if argv else 64, int(argv[1]) if len(argv) > 1 else 16, argv[2] if len(argv) > 2 else "bf16")
