"""The latent probe (air.metrics.LatentProbe, air_latent_probe) beside a torch fp64 formulation and the evaluation it follows.

  python tools/bench_latent_probe.py [M ...]
      For every M (default 1000 2000) at Z = 50, k = 5, 10 classes -- what an evaluation of training.py --latent-probe
      scores: up to two digits of 1000 test images -- 50 eager air_latent_probe calls (four launches); the same neighbours by
      torch in fp64 (the difference tensor squared and summed over z, then topk: an outside yardstick, NOT the stated
      arithmetic -- its sum has torch's order and its ties topk's); and 50 reset() + update() + score() + values(), what an
      evaluation enqueues, on a stub pass whose objects sit on the digits.  Prints HIP-event times; meant to run under
      `rocprofv3 --kernel-trace --stats` in a run of its own for the launch times (tools/rocprof_summary.py)."""
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import latent_probe_cases as pc
from air.metrics import LatentProbe, _ProbeBuffers

dev = torch.device("cuda", 0)
Z, K, CLASSES, CANVAS, WINDOW = 50, 5, 10, 50, 28


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


def stub_pass(case, G=2):
    """a pass of M / G images with G digits each whose objects sit on the digits: every digit is matched"""
    M = len(case["x"])
    B, T = M // G, 3
    att = np.zeros((T, B, 16), np.float32)
    ml = np.zeros((T, B, 2 * Z), np.float32)
    pos, box = np.zeros((B, G, 2), np.int32), np.zeros((B, G, 2), np.int32)
    for g in range(G):
        pos[:, g], box[:, g] = (5 + 20 * g, 7), (10, 12)
        att[g, :, 1] = ((5 + 20 * g) * 2 + 10 - 1.0) / 2.0 / ((CANVAS - 1) / 2.0) - 1.0
        att[g, :, 2] = (7 * 2 + 12 - 1.0) / 2.0 / ((CANVAS - 1) / 2.0) - 1.0
        ml[g, :, :Z] = case["x"][g::G]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                # noqa: E731
    model = types.SimpleNamespace(max_steps=T, batch_size=B, canvas_size=CANVAS, windows_size=WINDOW, vae_latent_dimensions=Z,
                                  input_images=torch.zeros(B, CANVAS ** 2, device=dev), att=up(att), ml=up(ml),
                                  run_digits=torch.full((B,), G, dtype=torch.int32, device=dev),
                                  vrec=torch.zeros(T, B, WINDOW * WINDOW, device=dev), _ensure=lambda: None)
    truth = (torch.full((B,), G, dtype=torch.int32, device=dev), up(pos), up(box), up(case["labels"].reshape(B, G)))
    return model, truth


def main(sizes):
    for M in sizes:
        case = pc.gaussian(M, Z, K, CLASSES, seed=1, spread=4.0)
        x, labels = torch.from_numpy(case["x"]).to(dev), torch.from_numpy(case["labels"]).to(dev)
        buffers = _ProbeBuffers("bench", dev, M, Z, K, CLASSES, 0.01, True).allocate()
        t_probe = timed(lambda: buffers.run(x, labels))
        res = buffers.summary()

        def by_torch():
            xd = x.double()
            d2 = (xd[:, None, :] - xd[None, :, :]).pow(2).sum(-1)
            d2.fill_diagonal_(float("inf"))
            return d2.topk(K, dim=1, largest=False)
        t_torch = timed(by_torch)
        same = float((by_torch()[1].sort(dim=1)[0] == buffers.neighbours.long().sort(dim=1)[0]).double().mean())
        model, truth = stub_pass(case)
        probe = LatentProbe(model, 2, classes=CLASSES, k=K)

        def evaluation():
            probe.reset()
            probe.update(*truth)
            probe.score()
            probe.values()
        t_eval = timed(evaluation)
        got = probe.result()
        print("latent probe, M = %d, Z = %d, k = %d: %.1f us per air_latent_probe (four launches, eager, HIP events); torch "
              "fp64 difference tensor + topk: %.1f us (%.4f of its neighbour sets are the probe's); %.1f us per reset() + "
              "update() + score() + values()" % (M, Z, K, t_probe, t_torch, same, t_eval))
        print("  knn_accuracy %.4f active_units %d scored %d; through the module: knn_accuracy %.4f scored %d matched %d of %d" % (
            res["knn_accuracy"], res["active_units"], res["scored"], got["knn_accuracy"], got["scored"], got["matched"], got["present"]))


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [1000, 2000])
