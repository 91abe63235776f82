"""The latent clusters (air.metrics.LatentClusters, air_latent_kmeans) at the size an evaluation scores.

  python tools/bench_latent_kmeans.py [M ...]
      For every M (default 2000) at Z = 50, k = 10, 10 classes, R = 8 restarts, at most 50 iterations -- what an evaluation of
      training.py --latent-clusters scores: up to two digits of 1000 test images -- 20 eager air_latent_kmeans calls (three
      launches) on Gaussian class blobs wide enough to overlap, and 20 reset() + update() + score() + values(), what an
      evaluation enqueues, on a stub pass whose objects sit on the digits (tools/bench_latent_probe.py's).  Prints HIP-event
      times; meant to run under `rocprofv3 --kernel-trace --stats` in a run of its own for the launch times
      (tools/rocprof_summary.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch

import latent_probe_cases as pc
from air.metrics import LatentClusters, _KMeansBuffers
from bench_latent_probe import stub_pass, timed

dev = torch.device("cuda", 0)
Z, K, CLASSES, RESTARTS, MAX_ITERS = 50, 10, 10, 8, 50


def main(sizes):
    for M in sizes:
        case = pc.gaussian(M, Z, 5, CLASSES, seed=1, spread=4.0)
        x, labels = torch.from_numpy(case["x"]).to(dev), torch.from_numpy(case["labels"]).to(dev)
        buffers = _KMeansBuffers("bench", dev, M, Z, K, CLASSES, RESTARTS, MAX_ITERS, 0, True).allocate()
        t_call = timed(lambda: buffers.run(x, labels), n=20)
        res = buffers.summary()
        model, truth = stub_pass(case)
        clu = LatentClusters(model, 2, classes=CLASSES, clusters=K, restarts=RESTARTS, max_iters=MAX_ITERS)

        def evaluation():
            clu.reset()
            clu.update(*truth)
            clu.score()
            clu.values()
        t_eval = timed(evaluation, n=20)
        got = clu.result()
        print("latent clusters, M = %d, Z = %d, k = %d, R = %d: %.1f us per air_latent_kmeans (three launches, eager, HIP events); "
              "%.1f us per reset() + update() + score() + values()" % (M, Z, K, RESTARTS, t_call, t_eval))
        print("  iterations per restart %s, %d converged, best %d; accuracy %.4f ari %.4f nmi %.4f live %d; through the module: "
              "accuracy %.4f scored %d matched %d of %d" % (
                  res["restart_iters"].tolist(), res["restarts_converged"], res["best"], res["accuracy"], res["ari"], res["nmi"],
                  res["live"], got["accuracy"], got["scored"], got["matched"], got["present"]))


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [2000])
