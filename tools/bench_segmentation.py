"""The segmentation metrics (air.metrics.Segmentation, air_segmentation) beside air_render at the same shape: the render
kernel does the same staging and the same per-pixel walk, so it is the yardstick of seg_image_kernel.

  python tools/bench_segmentation.py [k]
      50 eager air_render calls and 50 eager update() calls on k (default 1000) images of random records, windows and
      label planes at (T, G) = (3, 2) on the training driver's canvas (C = 50, w = 28) and on the largest one (C = 128,
      w = 32); then 50 reset() + update() + values(), what an evaluation of training.py --segmentation enqueues, and 50
      air_scene_masks launches.  Prints HIP-event times; meant to run under `rocprofv3 --kernel-trace --stats` in a run of
      its own for the launch times (tools/rocprof_summary.py)."""
import ctypes as C
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import segmentation_cases as sc
from air import _hip as H
from air.metrics import Segmentation

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
    T, G = 3, 2
    for Cc, w in ((50, 28), (128, 32)):
        ch = sc.random_chunk(np.random.RandomState(Cc), T, k, k, G, Cc, w)
        up = lambda a: torch.from_numpy(a).to(dev)                                  # noqa: E731
        model = types.SimpleNamespace(max_steps=T, batch_size=k, canvas_size=Cc, windows_size=w,
                                      input_images=torch.zeros(k, Cc * Cc, device=dev), att=up(ch["att"]), vrec=up(ch["vrec"]),
                                      _ensure=lambda: None)
        planes = up(ch["gt_mask"])
        canvas = torch.zeros(k, Cc * Cc, device=dev)
        digits = torch.zeros(k, dtype=torch.int32, device=dev)
        r = H.Render(H.ptr(model.vrec), H.ptr(model.att), H.ptr(canvas), H.ptr(digits), k, T, Cc, w)
        t_render = timed(lambda: H.launch("air_render", dev, C.byref(r)))
        seg = Segmentation(model, G, keep=True)
        t_update = timed(lambda: seg.update(planes))
        lean = Segmentation(model, G)
        t_lean = timed(lambda: lean.update(planes))

        def evaluation():
            lean.reset()
            lean.update(planes)
            lean.values()
        t_eval = timed(evaluation)
        res = lean.result()
        print("segmentation, T = %d, G = %d, k = %d, C = %d, w = %d: air_render %.1f us; update() %.1f us with every output kept, "
              "%.1f us with none (two launches, eager, HIP events); %.1f us per reset() + update() + values()"
              % (T, G, k, Cc, w, t_render, t_update, t_lean, t_eval))
        print("  last evaluation: scored %d present %d fg_pixels %d fg_ari %.4f mask_iou %.4f" % (
            res["scored"], res["present"], res["fg_pixels"], res["fg_ari"], res["mask_iou"]))
        # air_scene_masks on the same canvas: 100 glyphs of 28 x 28, two digits a scene
        rng = np.random.RandomState(1)
        glyphs = (rng.uniform(0, 1, (100, 28 * 28)) * (rng.uniform(0, 1, (100, 28 * 28)) < 0.3)).astype(np.float32)
        arrays = dict(glyphs=up(glyphs), crops=up(np.tile(np.asarray([[4, 4, 20, 20]], np.int32), (100, 1))),
                      indices=up(rng.randint(0, 100, (k, 2)).astype(np.int32)),
                      positions=up(rng.randint(0, Cc - 20, (k, 4)).astype(np.int32)), canvas_dim=Cc)
        count = up(rng.randint(0, 3, k).astype(np.int32))
        t_masks = timed(lambda: Segmentation.scene_masks(arrays, count))
        print("  scene_masks, B = %d, C = %d: %.1f us (one launch + the allocation of its output)" % (k, Cc, t_masks))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 1000)
