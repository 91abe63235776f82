"""The localisation metrics (air.metrics.Localization, air_localization) beside the evaluation forward they follow.

  python tools/bench_localization.py [k]
      50 eager update() calls on k (default 1000) images of random records and boxes at (T, G) = (3, 2), the training
      driver's test model, and at the limits (16, 16); then 50 reset() + update() + values(), what an evaluation of
      training.py --localization enqueues.  Prints HIP-event times; meant to run under `rocprofv3 --kernel-trace --stats`
      in a run of its own for the launch times (tools/rocprof_summary.py)."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import localization_cases as lc
from air.metrics import Localization

dev = torch.device("cuda", 0)


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


def main(k):
    for T, G in ((3, 2), (16, 16)):
        case = lc.random_case(1, (k,), T, k, G)
        ch = case["chunks"][0]
        up = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
        model = types.SimpleNamespace(max_steps=T, batch_size=k, canvas_size=50, input_images=torch.zeros(k, 2500, device=dev),
                                      att=up(ch["att"]), run_digits=up(ch["run_digits"]), _ensure=lambda: None)
        truth = tuple(up(ch[n]) for n in ("gt_count", "gt_positions", "gt_boxes"))
        loc = Localization(model, G)
        t_update = timed(lambda: loc.update(*truth))

        def evaluation():
            loc.reset()
            loc.update(*truth)
            loc.values()
        t_eval = timed(evaluation)
        res = loc.result()
        print("localization, T = %d, G = %d, k = %d: %.1f us per update() (two launches, eager, HIP events); %.1f us per "
              "reset() + update() + values()" % (T, G, k, t_update, t_eval))
        print("  last evaluation: present %d inferred %d matched %d hits %d mean_iou %.4f" % (
            res["present"], res["inferred"], res["matched"], res["hits"], res["mean_iou"]))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1000)
