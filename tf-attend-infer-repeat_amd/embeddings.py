"""Counterpart of the reference's embeddings.py: restores a trained model, runs it over test.tfrecords, matches the digits it
found to the ground truth and writes what TensorBoard's embedding projector opens (metadata, sprite sheet, a checkpoint with
the latents as variable `air_mnist`, an event file, projector_config.pbtxt).

  python embeddings.py --model air_results/models/air-model-60000.pt [--data multi_mnist_data/test.tfrecords]
                       [--out ./embeddings] [--max-distance 0.2] [--precision fp32] [--batch-size 64]

  tensorboard --logdir ./embeddings

The match, the gathering of latents and windows and the sprite sheet run on the device (air/embeddings.py).  The reference
also reads MNIST, only to print a line; that is left out.
"""
import argparse
import os
import shutil

import torch

from air import embeddings
from air.air_model import AIRModel, saved_cnn_arguments
from multi_mnist import read_test_data

CANVAS_SIZE = 50
WINDOW_SIZE = 28
MODEL_PATH = "./air_results/models/air-model-0.pt"
TEST_DATA_FILE = "multi_mnist_data/test.tfrecords"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default=MODEL_PATH, help=".pt state dict, or the prefix of a TensorFlow bundle")
    ap.add_argument("--data", default=TEST_DATA_FILE)
    ap.add_argument("--out", default="./embeddings", help="removed and re-created")
    ap.add_argument("--max-distance", type=float, default=0.2)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--batch-size", type=int, default=64)
    args = ap.parse_args()

    out = os.path.abspath(args.out)
    shutil.rmtree(out, ignore_errors=True)                                          # embeddings.py:145-146
    os.makedirs(out)

    dev = torch.device("cuda", 0)
    B = args.batch_size
    print("Creating model...")
    air_model = AIRModel(                                                           # embeddings.py:153-160
        torch.zeros(B, CANVAS_SIZE ** 2, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
        max_steps=3, rnn_units=256, canvas_size=CANVAS_SIZE, windows_size=WINDOW_SIZE,
        vae_latent_dimensions=50, vae_recognition_units=(512, 256), vae_generative_units=(256, 512),
        vae_likelihood_std=0.3, scale_hidden_units=64, shift_hidden_units=64, z_pres_hidden_units=64,
        z_pres_temperature=1.0, stopping_threshold=0.99, **saved_cnn_arguments(args.model),
        train=False, reuse=False, scope="air", gemm_precision=args.precision,
    )
    print("Restoring model...")
    if os.path.exists(args.model + ".index"):                 # a TensorFlow bundle (the reference's model/air-model)
        air_model.load_tf_checkpoint(args.model)
    else:
        air_model.load_state_dict(torch.load(args.model, map_location="cpu"), load_optimizer=False)

    print("Reading AIR data...")
    data = read_test_data(args.data)
    print("Matching original AIR data with reconstructions...")
    result = embeddings.collect(air_model, *data, max_distance=args.max_distance)

    label_dic = {d: 0 for d in range(10)}
    for label in result.labels.cpu().tolist():
        label_dic[label] = label_dic.get(label, 0) + 1
    print()
    print("Present digits: {0}".format(result.present))
    print("Inferred digits: {0}".format(result.inferred))
    print("Matched inference boxes: {0}".format(result.matched))
    print("Digit distribution (among matched digits):")
    print(label_dic)
    print()

    if result.matched == 0:
        raise SystemExit("no inferred object lies within %g of a ground-truth digit: nothing to export" % args.max_distance)
    print("Saving embeddings...")
    embeddings.write_projector(out, result)


if __name__ == "__main__":
    main()
