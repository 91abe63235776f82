"""Counterpart of the reference's embeddings.py: restores a trained model, runs it over test.tfrecords, matches the digits it
found to the ground truth and writes what TensorBoard's embedding projector opens (metadata, sprite sheet, a checkpoint with
the latents as variable `air_mnist`, an event file, projector_config.pbtxt).

  python embeddings.py --model air_results/models/air-model-60000.pt [--data multi_mnist_data/test.tfrecords]
                       [--out ./embeddings] [--max-distance 0.2] [--precision fp32] [--batch-size 64] [--knn 5] [--kmeans 10]

  tensorboard --logdir ./embeddings

The match, the gathering of latents and windows and the sprite sheet run on the device (air/embeddings.py).  The reference
also reads MNIST, only to print a line; that is left out.  --knn K scores what the projector shows as numbers
(air.embeddings.probe: leave-one-out K-nearest-neighbour digit accuracy, confusion matrix, active units) and writes
latent_probe.json beside the projector files.  --kmeans K asks whether the classes emerge without labels
(air.embeddings.cluster: exact K-means over the matched latents, every cluster mapped to its majority class): it prints
clustering accuracy, adjusted Rand index and NMI, and writes clusters.npz and cluster_sprites.png, the decoder's window of
every centroid that has members.
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
    ap.add_argument("--knn", type=int, default=0, metavar="K",
                    help="also score the matched latents: leave-one-out K-nearest-neighbour digit accuracy, its confusion "
                         "matrix and the active units (air.embeddings.probe), printed and written to latent_probe.json")
    ap.add_argument("--kmeans", type=int, default=0, metavar="K",
                    help="also cluster the matched latents without their labels: exact K-means, clustering accuracy, adjusted "
                         "Rand index and NMI against the digit labels (air.embeddings.cluster), printed and written to "
                         "clusters.npz, with cluster_sprites.png: what the decoder draws for every centroid")
    ap.add_argument("--kmeans-restarts", type=int, default=8, metavar="R", help="--kmeans: the seeded starts (1 .. 32)")
    ap.add_argument("--kmeans-seed", type=int, default=0, help="--kmeans: the seed of the starts")
    args = ap.parse_args()
    if args.knn < 0 or args.knn > 16:
        ap.error("--knn must lie in [1, 16] (0: no probe)")
    if args.kmeans < 0 or args.kmeans > 64:
        ap.error("--kmeans must lie in [1, 64] (0: no clustering)")
    if args.kmeans and not 1 <= args.kmeans_restarts <= 32:
        ap.error("--kmeans-restarts must lie in [1, 32]")

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
    probed = None
    if args.knn:
        probed = embeddings.probe(result, k=args.knn, classes=max(10, max(label_dic) + 1))
        print("Latent probe (leave-one-out {0}-NN over {1} matched digits):".format(args.knn, probed["scored"]))
        print("k-NN digit accuracy: {0:.4f}".format(probed["knn_accuracy"]))
        print("Active units (variance > {0:g}): {1} of {2}".format(probed["au_threshold"], probed["active_units"], len(probed["mean"])))
        print("Confusion matrix (rows: true digit, columns: predicted):")
        print(probed["confusion"])
        print()
    clustered = None
    if args.kmeans:
        clustered = embeddings.cluster(result.latents, result.labels, clusters=args.kmeans, classes=max(10, max(label_dic) + 1),
                                       restarts=args.kmeans_restarts, seed=args.kmeans_seed)
        print("Latent clusters ({0}-means, {1} restarts, best {2} after {3} iterations{4}, over {5} matched digits):".format(
            args.kmeans, args.kmeans_restarts, clustered["best"], clustered["iters"],
            "" if clustered["converged"] else ", not converged", clustered["labelled"]))
        print("Clustering accuracy: {0:.4f}  ARI: {1:.4f}  NMI: {2:.4f}  live clusters: {3}".format(
            clustered["accuracy"], clustered["ari"], clustered["nmi"], clustered["live"]))
        print("Cluster table (rows: cluster, columns: true digit):")
        print(clustered["table"])
        print()
    print("Saving embeddings...")
    embeddings.write_projector(out, result)
    if clustered is not None:
        embeddings.write_clusters(out, clustered, air_model)
    if probed is not None:
        embeddings.write_probe(out, probed)


if __name__ == "__main__":
    main()
