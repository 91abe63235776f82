"""The glyph bank (multi_mnist.DeviceGlyphBank) beside the scene source it feeds (tools/bench_scene_source.py has the source
beside the queue).

  python tools/bench_glyph_bank.py launch [variants]
      50 eager refreshes of a bank of `variants` (default 4096) jittered glyphs of the stand-in set (gd = 28, od = 32,
      0.9-1.1, +-15 degrees).  Prints the HIP-event time per refresh and the status counts of the last bank; meant to run
      under `rocprofv3 --kernel-trace --stats` in a run of its own for the launch time (tools/rocprof_summary.py).
  python tools/bench_glyph_bank.py step [steps per replay] [rounds] [variants]
      ms per train step of the training driver's replay (bf16, bench.py's model) with the plain source's hooks and with a
      source on a bank that the replay refreshes first, alternating, `rounds` times each."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch

import multi_mnist as mm

dev = torch.device("cuda", 0)
JITTER = dict(min_w=0.9, max_w=1.1, min_h=0.9, max_h=1.1, min_ang=-15.0, max_ang=15.0)


def launch(V):
    bank = mm.DeviceGlyphBank(mm.load_glyphs()[0], V, seed=1, device=dev, **JITTER)
    for _ in range(5):
        bank.refresh()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50
    e0.record()
    for _ in range(n):
        bank.refresh()
    e1.record()
    torch.cuda.synchronize()
    print("glyph bank, V = %d, gd = %d, od = %d: %.1f us per refresh (jitter + advance, eager, HIP events)" % (
        V, bank.gd, bank.od, e0.elapsed_time(e1) * 1e3 / n))
    print("  status of the last bank (usable, empty, too large): %s; boxes up to %s" % (
        bank.status_counts().tolist(), bank.bank_crops[:, 2:].max(0).values.tolist()))


def step(G, rounds, V):
    from bench import ANNEAL, HP
    from air import air_model as am
    glyphs = mm.load_glyphs()[0]
    res = {"source": [], "bank": []}
    for r in range(rounds):
        for tag in res:
            x, t = torch.zeros(64, 2500, device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
            bank = mm.DeviceGlyphBank(glyphs, V, seed=1 + r, device=dev, **JITTER) if tag == "bank" else None
            feed = mm.DeviceSceneSource(glyphs if bank is None else bank, 64, x, t, seed=1 + r)
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
            print("round %d  %-6s %.4f ms per step, %d canvases given up" % (r, tag, res[tag][-1], int(feed.gave_up())), flush=True)
            m.release_graph()
    for tag, v in res.items():
        print("%-6s median %.4f  min %.4f  max %.4f ms per step (%d steps per replay, %d rounds, %d variants)" % (
            tag, sorted(v)[len(v) // 2], min(v), max(v), G, rounds, V))


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    if (sys.argv[1] if len(sys.argv) > 1 else "launch") == "launch":
        launch(arg(2, 4096))
    else:
        step(arg(2, 50), arg(3, 3), arg(4, 4096))
