"""Headless counterpart of the reference's demo.py: restores a trained model, runs inference on a
set of canvases and writes what the tkinter demo / the TensorBoard image summary would show --
one PNG grid of [original + attention boxes | reconstruction + attention boxes] (like
images/rec_samples.png) and a JSON with the inferred digit counts and [s, x, y] positions.

  python demo.py --model air_results/models/air-model-60000.pt [--data multi_mnist_data/test.npz]
                 [--num-images 60] [--out demo_out]

  python demo.py --model ... --generate 16 [--out demo_out]

--generate N needs no data: N scenes are drawn from the model's priors and rendered on the device (AIRModel.generate);
it writes generated_samples.png ([scene | scene + attention boxes]) and generated.json.

--segmentation also writes segmentation_samples.png: [input | predicted instance masks], every pixel in the colour of the
object that explains it (air.metrics.Segmentation; red, green, blue for the first, second, third step).

The interactive tkinter window (demo/demo_window.py, pixel_canvas.py) is out of scope.
"""
import argparse
import json
import os

import numpy as np
import torch

from air.air_model import AIRModel, saved_cnn_arguments
from air.visualize import colour_masks, save_image_grid, visualize_reconstructions, visualize_scenes
from demo.model_wrapper import ModelWrapper

CANVAS_SIZE = 50
WINDOW_SIZE = 28
MODEL_PATH = "./air_results/models/air-model-0.pt"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=MODEL_PATH)
    ap.add_argument("--data", default="", help=".npz with `images` [n,2500] (default: a freshly generated test set)")
    ap.add_argument("--num-images", type=int, default=60)
    ap.add_argument("--out", default="demo_out")
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--generate", type=int, default=0, metavar="N",
                    help="draw N scenes from the model's priors instead of running inference (no data needed)")
    ap.add_argument("--seed", type=int, default=0, help="--generate: seed of the device noise stream")
    ap.add_argument("--prior-log-odds", type=float, default=None,
                    help="--generate: z_pres prior log-odds (default: the model's constructor value)")
    ap.add_argument("--segmentation", action="store_true",
                    help="also write segmentation_samples.png: the inputs beside the predicted instance masks")
    ap.add_argument("--segmentation-threshold", type=float, default=0.5,
                    help="--segmentation: an object claims a pixel where its part of the reconstruction is above this")
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    if args.generate > 0:
        images, targets = np.zeros((args.generate, CANVAS_SIZE ** 2), np.float32), np.zeros(args.generate, np.int32)
    elif args.data:
        d = np.load(args.data)
        images = d["images"][:args.num_images].astype(np.float32)
        targets = d["digits"][:args.num_images].astype(np.int32) if "digits" in d else np.zeros(len(images), np.int32)
    else:
        from multi_mnist import generate_dataset
        ds = generate_dataset(images_per_digit=max(args.num_images, 30), test_set_size=args.num_images, seed=1)
        images, targets = ds["test_images"], ds["test_digits"]
    n = len(images)

    test_data = torch.zeros(n, CANVAS_SIZE ** 2, device=dev)
    test_targets = torch.tensor(targets, dtype=torch.int32, device=dev)
    print("Creating model...")
    air_model = AIRModel(                                                           # demo.py:19-27
        test_data, test_targets,
        max_steps=3, rnn_units=256, canvas_size=CANVAS_SIZE, windows_size=WINDOW_SIZE,
        vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
        vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
        z_pres_temperature=1.0, stopping_threshold=0.99, **saved_cnn_arguments(args.model),
        train=False, reuse=False, scope="air", gemm_precision=args.precision, seed=args.seed,
    )
    print("Restoring model...")
    if os.path.exists(args.model + ".index"):                 # a TensorFlow bundle (the reference's model/air-model)
        air_model.load_tf_checkpoint(args.model)
    else:
        air_model.load_state_dict(torch.load(args.model, map_location="cpu"), load_optimizer=False)   # inference: variables only
    wrapper = ModelWrapper(air_model, None, test_data, CANVAS_SIZE, WINDOW_SIZE)

    if args.generate > 0:
        return generate(args, air_model, wrapper, dev)
    digits, positions, recs, windows, latents, loss = wrapper.infer(list(images))
    os.makedirs(args.out, exist_ok=True)
    vis = visualize_reconstructions(air_model.input_images, air_model.reconstruction, air_model.rec_st_back,
                                    air_model.rec_num_digits, CANVAS_SIZE, WINDOW_SIZE, air_model.max_steps, zoom=2)
    png = save_image_grid(vis, os.path.join(args.out, "rec_samples.png"), columns=10)
    rows = [{"image": i, "target_digits": int(targets[i]), "inferred_digits": int(digits[i]),
             "positions_s_x_y": [[round(float(v), 4) for v in p] for p in positions[i]],
             "reconstruction_loss": round(float(loss[i]), 3)} for i in range(n)]
    with open(os.path.join(args.out, "inference.json"), "w") as f:
        json.dump(rows, f, indent=1)
    acc = float(np.mean([r["target_digits"] == r["inferred_digits"] for r in rows]))
    print("wrote %s and inference.json (%d images, digit-count accuracy %.3f)" % (png, n, acc))
    if args.segmentation:
        from air.metrics import Segmentation
        seg = Segmentation(air_model, 1, pred_threshold=args.segmentation_threshold, keep=True)
        seg.update(torch.zeros(n, CANVAS_SIZE ** 2, dtype=torch.uint8, device=dev))      # (no truth here: the labels are the point)
        plain = air_model.input_images.reshape(n, CANVAS_SIZE, CANVAS_SIZE)
        left = torch.stack([plain, plain, plain], dim=3)
        stripe = torch.ones(n, CANVAS_SIZE, 2, 3, device=dev)
        grid = torch.cat([left, stripe, colour_masks(seg.pred_mask, air_model.input_images)], dim=2)
        print("wrote %s" % save_image_grid(grid, os.path.join(args.out, "segmentation_samples.png"), columns=10))


def generate(args, air_model, wrapper, dev):
    n, N = args.generate, air_model.max_steps
    if args.prior_log_odds is not None:
        air_model.set_dynamic(z_pres_prior_log_odds=args.prior_log_odds)
    digits, positions, canvases, windows, latents = wrapper.generate(n)
    os.makedirs(args.out, exist_ok=True)
    # the window -> canvas matrices (air_model.py:353-356) of every scene's objects, from the returned [s, x, y] rows
    st = np.zeros((n, N, 2, 3), np.float32)
    for i, p in enumerate(positions):
        for t in range(digits[i]):
            s, x, y = (float(v) for v in p[t])
            st[i, t] = [[1.0 / s, 0.0, -x / s], [0.0, 1.0 / s, -y / s]]
    vis = visualize_scenes(torch.tensor(np.stack(canvases).reshape(n, -1), device=dev), torch.tensor(st, device=dev),
                           torch.tensor(digits, dtype=torch.int32, device=dev), CANVAS_SIZE, WINDOW_SIZE, N, zoom=2)
    png = save_image_grid(vis, os.path.join(args.out, "generated_samples.png"), columns=min(8, n))
    rows = [{"scene": i, "objects": int(digits[i]),
             "positions_s_x_y": [[round(float(v), 4) for v in p] for p in positions[i]]} for i in range(n)]
    with open(os.path.join(args.out, "generated.json"), "w") as f:
        json.dump(rows, f, indent=1)
    print("wrote %s and generated.json (%d scenes, %.2f objects per scene)" % (png, n, float(np.mean(digits))))


if __name__ == "__main__":
    main()
