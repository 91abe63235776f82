"""Wall time of the projector export's middle on a 2 000-image test set (B = 64, fp32), two ways, in one process:

  device   air.embeddings.collect() + sprite_sheet() + the read-back of latents, labels, ids and the uint8 sheet
  today    what a user could do before: ModelWrapper.infer on the same images (every window, latent and reconstruction
           copied to the host, chunk by chunk) followed by the Python restatement of the match and of the sprite levels
           (tests/embedding_cases.py) -- existing code plus the test restatement, never the code under test

The test set is generate_dataset's (strata of 0, 1, 2 digits shuffled together), taken through generate_strata because only
that returns the ground truth.  The model is freshly initialised with the z_pres bias raised until it finds objects; its
device noise is keyed by (seed, global step), the same in every forward, so both paths see the same objects and the bench
asserts that they produce the same bytes.  An untrained model's shifts land near a digit by chance only: --max-distance 0.2
matches few digits, --max-distance 1.0 most of them (the share a trained model reaches at 0.2); both are worth a run.

One warm-up of each path, then three repeats alternating them; host clock around work that ends in a synchronise.
    python tools/bench_embeddings.py [--max-distance 0.2] [--images 2000] [--profile]
--profile: the device path alone, twice (for rocprofv3 --kernel-trace --stats, in a run of its own)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tf-attend-infer-repeat_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch
import embedding_cases as ec
from air import air_model as am, embeddings
from demo.model_wrapper import ModelWrapper
from multi_mnist import generate_strata

ap = argparse.ArgumentParser()
ap.add_argument("--max-distance", type=float, default=0.2)
ap.add_argument("--images", type=int, default=2000)
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()
B, n = 64, args.images

strata, rng, source = generate_strata(2, -(-n // 3), seed=0)
keys = ("images", "digits", "indices", "positions", "boxes", "labels")
perm = rng.permutation(sum(len(st["images"]) for st in strata))[:n]
data = [[v for st in strata for v in st[k]] for k in keys]
images, digits, indices, positions, boxes, labels = ([col[i] for i in perm] for col in data)

model = am.AIRModel(torch.zeros(B, 2500, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda"),
                    max_steps=3, rnn_units=256, canvas_size=50, windows_size=28,
                    vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                    vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                    z_pres_temperature=1.0, stopping_threshold=0.99, cnn=False, train=False, scope="air", gemm_precision="fp32")
sd = model.state_dict()
bias = [k for k in sd if k.endswith("z_pres/log_odds/output/biases")][0]
sd[bias] = sd[bias] + 3.0
model.load_state_dict(sd, load_optimizer=False)
wrapper = ModelWrapper(model, None, None)


def device_path():
    res = embeddings.collect(model, images, digits, indices, positions, boxes, labels, max_distance=args.max_distance)
    sheet = embeddings.sprite_sheet(res.windows)
    out = (res.latents.cpu().numpy(), res.labels.cpu().numpy(), res.ids.cpu().numpy(), sheet.cpu().numpy())   # (synchronises)
    return res, out


def today_path():
    rec = wrapper.infer(images)
    got = ec.collect_lists(digits, indices, positions, boxes, labels, rec[0], rec[1], rec[3], rec[4], max_distance=args.max_distance)
    return got, ec.sprite_levels(got["windows"])


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


if args.profile:
    for _ in range(2):
        device_path()
    torch.cuda.synchronize()
    sys.exit(0)

(_, (res, out)), (_, (got, sheet)) = wall(device_path), wall(today_path)       # warm-up, and: the same bytes
assert (res.present, res.inferred, res.matched) == (got["present"], got["inferred"], got["matched"]) and res.matched > 0
assert out[0].tobytes() == got["latents"].tobytes() and out[1].tobytes() == got["labels"].tobytes()
assert out[2].tobytes() == got["ids"].tobytes() and out[3].tobytes() == sheet.tobytes()
assert res.windows.cpu().numpy().tobytes() == got["windows"].tobytes()
times = {"device": [], "today": []}
for _ in range(3):
    times["device"].append(wall(device_path)[0])
    times["today"].append(wall(today_path)[0])
med = {k: sorted(v)[1] * 1e3 for k, v in times.items()}
spread = {k: (max(v) - min(v)) / sorted(v)[1] for k, v in times.items()}
print("%d images (%s glyphs), B = %d, max_distance %g: present %d inferred %d matched %d; device path %.1f ms, infer + Python "
      "restatement %.1f ms (medians of 3, alternating; spread %.0f%% / %.0f%%)" %
      (n, source, B, args.max_distance, res.present, res.inferred, res.matched, med["device"], med["today"],
       100 * spread["device"], 100 * spread["today"]), flush=True)
print(json.dumps({"images": n, "batch": B, "max_distance": args.max_distance, "matched": res.matched, "present": res.present,
                  "inferred": res.inferred, "median_ms": med, "spread": spread, "all_ms": {k: [x * 1e3 for x in v] for k, v in times.items()}}))
