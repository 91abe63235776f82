"""The scene source (multi_mnist.DeviceSceneSource) beside the device queue (ShuffleBatchQueue) it can replace.

  python tools/bench_scene_source.py launch [small|large]
      200 eager batches of the source -- small: B = 64, 50 x 50, 0-2 digits; large: B = 256, 128 x 128, 0-4 digits -- and,
      with `small`, 200 eager dequeue + gather batches of the queue at the same shape.  Prints HIP-event times per batch;
      meant to run under `rocprofv3 --kernel-trace --stats` in a run of its own for the per-launch times
      (tools/rocprof_summary.py makes the table).
  python tools/bench_scene_source.py step [steps per replay] [rounds]
      ms per train step of the training driver's replay (bf16, bench.py's model) with the queue's hooks and with the
      source's, alternating, `rounds` times each."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch

import multi_mnist as mm

dev = torch.device("cuda", 0)


def _events(fn, n=200, warm=10):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def launch(which):
    glyphs = mm.load_glyphs()[0]
    B, Cn, md = (64, 50, 2) if which == "small" else (256, 128, 4)
    x, t = torch.zeros(B, Cn * Cn, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    src = mm.DeviceSceneSource(glyphs, B, x, t, canvas_dim=Cn, max_digits=md, seed=1)
    print("scene source, B = %d, %d x %d, 0-%d digits: %.2f us per batch (compose + advance, eager, HIP events)" % (
        B, Cn, Cn, md, _events(src.next_batch)))
    print("  given up: %d of %d canvases; restarted in the last batch: %d" % (
        int(src.gave_up()), int(src.counter) * B, int((src.status > 0).sum())))
    if which == "small":
        from bench import synthetic_canvases
        im, tg = synthetic_canvases(12000, Cn, md, 1)
        q = mm.ShuffleBatchQueue(torch.tensor(im, device=dev), torch.tensor(tg, device=dev), B, x, t, seed=1)
        print("queue, B = %d, %d x %d: %.2f us per batch (dequeue + gather, eager, HIP events)" % (B, Cn, Cn, _events(q.next_batch)))


def step(G, rounds):
    from bench import ANNEAL, HP, synthetic_canvases
    from air import air_model as am
    im, tg = synthetic_canvases(12000, 50, 2, 1)
    images, digits = torch.tensor(im, device=dev), torch.tensor(tg, device=dev)
    glyphs = mm.load_glyphs()[0]
    res = {"queue": [], "source": []}
    for r in range(rounds):
        for tag in ("queue", "source"):
            x, t = torch.zeros(64, 2500, device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
            if tag == "queue":
                feed = mm.ShuffleBatchQueue(images, digits, 64, x, t, seed=1 + r)
            else:
                feed = mm.DeviceSceneSource(glyphs, 64, x, t, seed=1 + r)
            am.reset_default_graph()
            m = am.AIRModel(x, t, cnn=False, train=True, annealing_schedules=ANNEAL, gemm_precision="bf16", **HP)
            between, after = feed.graph_hooks(G)
            m.capture_graph(steps=G, between_steps=between, after_steps=after)
            for _ in range(3):
                m.training()
            torch.cuda.synchronize()
            n = 40
            t0 = time.perf_counter()
            for _ in range(n):
                m.training()
            torch.cuda.synchronize()
            res[tag].append((time.perf_counter() - t0) / (n * G) * 1e3)
            print("round %d  %-6s %.4f ms per step" % (r, tag, res[tag][-1]), flush=True)
            m.release_graph()
    for tag, v in res.items():
        print("%-6s median %.4f  min %.4f  max %.4f ms per step (%d steps per replay, %d rounds)" % (
            tag, sorted(v)[len(v) // 2], min(v), max(v), G, rounds))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "launch"
    if mode == "launch":
        launch(sys.argv[2] if len(sys.argv) > 2 else "small")
    else:
        step(int(sys.argv[2]) if len(sys.argv) > 2 else 50, int(sys.argv[3]) if len(sys.argv) > 3 else 3)
