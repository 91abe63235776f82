"""The segmentation metrics on STAND-IN glyphs, offline: training.py composes no test set on the device for them, so
--segmentation is refused there.  This restores a checkpoint of a stand-in run into the driver's test model, composes scenes
with a stand-in DeviceSceneSource straight into its input buffer, takes their instance masks from Segmentation.scene_masks
and scores one inference pass with Segmentation and, beside it, Localization.  Prints one JSON line.

  python tools/segmentation_standin.py air_results/models/air-model-60000.pt [--scenes 1000] [--seed 0] [--threshold 0.5]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tf-attend-infer-repeat_amd"))
import torch

import multi_mnist as mm
from air.air_model import AIRModel, saved_cnn_arguments
from air.metrics import Localization, Segmentation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("model")
    ap.add_argument("--scenes", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--threshold", type=float, default=0.5)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, Cc, G = args.scenes, 50, 2
    images = torch.zeros(n, Cc * Cc, device=dev)
    digits = torch.zeros(n, dtype=torch.int32, device=dev)
    model = AIRModel(images, digits, max_steps=3, rnn_units=256, canvas_size=Cc, windows_size=28,
                     vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
                     vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
                     z_pres_temperature=1.0, stopping_threshold=0.99, **saved_cnn_arguments(args.model),
                     train=False, reuse=False, scope="air", gemm_precision=args.precision, seed=args.seed)
    model.load_state_dict(torch.load(args.model, map_location="cpu"), load_optimizer=False)
    source = mm.DeviceSceneSource(mm.load_glyphs()[0], n, images, digits, canvas_dim=Cc, max_digits=G, seed=0x5345474D + args.seed)
    source.next_batch()
    masks = Segmentation.scene_masks(source, digits)
    model.forward()
    seg = Segmentation(model, G, pred_threshold=args.threshold)
    seg.update(masks)
    loc = Localization(model, G)
    meta = source.meta()
    loc.update(digits, meta["positions"], meta["boxes"])
    s, l = seg.result(), loc.result()
    out = {"model": args.model, "glyph_style": "standin", "scenes": n, "seed": args.seed, "pred_threshold": args.threshold,
           "accuracy": round(l["count_accuracy"], 4),
           "segmentation": {k: round(s[k], 4) for k in Segmentation.names()},
           "localization": {k: round(l[k], 4) for k in Localization.names()},
           "totals": {k: s[k] for k in ("images", "scored", "present", "fg_pixels", "fg_missed_pixels", "bg_claimed_pixels")}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
