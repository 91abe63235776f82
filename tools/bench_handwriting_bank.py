"""The handwriting bank (multi_mnist.DeviceHandwritingBank, the MNIST_LIKE preset) beside the scene source it feeds
(tools/bench_glyph_bank.py has the jitter bank).

  python tools/bench_handwriting_bank.py launch [variants]
      50 eager refreshes of a bank of `variants` (default 4096) of the preset (gd = 40, ink = 20, od = 28).  Prints the
      HIP-event time per refresh and the status counts of the last bank; meant to run under `rocprofv3 --kernel-trace
      --stats` in a run of its own for the launch time (tools/rocprof_summary.py).
  python tools/bench_handwriting_bank.py step [steps per replay] [rounds] [variants]
      ms per train step of the training driver's replay (bf16, bench.py's model) with the plain source's hooks and with a
      source on a handwriting bank that the replay refreshes first, alternating, `rounds` times each.
  python tools/bench_handwriting_bank.py stats [variants]
      one bank of the preset read back: the share of unusable variants, box sizes, ink per glyph, and the stroke width
      (twice the ink area over the length of the ink's outline, the width of a long stroke of that area and outline)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import numpy as np
import torch

import multi_mnist as mm

dev = torch.device("cuda", 0)


def launch(V):
    bank, _ = mm.handwriting_bank(V, 1, dev)
    for _ in range(5):
        bank.refresh()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50
    e0.record()
    for _ in range(n):
        bank.refresh()
    e1.record()
    torch.cuda.synchronize()
    print("handwriting bank, V = %d, gd = %d, ink = %d, od = %d, radius = %d: %.1f us per refresh (distort + advance, eager, HIP events)" % (
        V, bank.gd, bank.ink, bank.od, bank.radius, e0.elapsed_time(e1) * 1e3 / n))
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
            bank = mm.handwriting_bank(V, 1 + r, dev)[0] if tag == "bank" else None
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


def stats(V):
    bank, _ = mm.handwriting_bank(V, 1, dev)
    bank.refresh()
    torch.cuda.synchronize()
    status, crops = bank.status.cpu().numpy(), bank.bank_crops.cpu().numpy()
    frames = bank.bank.cpu().numpy().reshape(V, bank.od, bank.od)
    ok = status == 0
    print("preset bank, V = %d: status counts %s, unusable share %.4f" % (V, np.bincount(status, minlength=3).tolist(), 1.0 - ok.mean()))
    w, h = crops[ok][:, 2], crops[ok][:, 3]
    print("  box: larger side == ink on %.4f of the usable; w mean %.2f (min %d, max %d), h mean %.2f (min %d, max %d)" % (
        (np.maximum(w, h) == bank.ink).mean(), w.mean(), w.min(), w.max(), h.mean(), h.min(), h.max()))
    ink = frames[ok] > 0
    pad = np.pad(ink, ((0, 0), (1, 1), (1, 1)))
    edges = sum((pad[:, 1:-1, 1:-1] & ~n).sum((1, 2)) for n in (pad[:, :-2, 1:-1], pad[:, 2:, 1:-1], pad[:, 1:-1, :-2], pad[:, 1:-1, 2:]))
    width = 2.0 * ink.sum((1, 2)) / edges
    sat = (frames[ok] >= 1.0).sum((1, 2)) / ink.sum((1, 2))
    print("  ink pixels per glyph: mean %.1f (min %d, max %d); saturated share of the ink %.3f; mean value of a frame %.4f" % (
        ink.sum((1, 2)).mean(), ink.sum((1, 2)).min(), ink.sum((1, 2)).max(), sat.mean(), frames[ok].mean()))
    print("  stroke width 2 * area / outline: mean %.2f px, 5th / 50th / 95th percentile %.2f / %.2f / %.2f" % (
        width.mean(), *np.percentile(width, [5, 50, 95])))
    n = bank.params[:, 6].cpu().numpy()[ok]
    for k in sorted(set(n)):
        print("    stroke passes %+d: %4d variants, width %.2f px" % (k, (n == k).sum(), width[n == k].mean()))


if __name__ == "__main__":
    arg = lambda i, d: int(sys.argv[i]) if len(sys.argv) > i else d
    mode = sys.argv[1] if len(sys.argv) > 1 else "launch"
    if mode == "launch":
        launch(arg(2, 4096))
    elif mode == "stats":
        stats(arg(2, 4096))
    else:
        step(arg(2, 50), arg(3, 3), arg(4, 4096))
