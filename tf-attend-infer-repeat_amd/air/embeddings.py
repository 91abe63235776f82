"""Projector export -- the middle of the reference's embeddings.py (:29-131) on the device.

``collect(model, *read_test_data(...))`` runs an inference ``AIRModel`` over a test set chunk by chunk and, after each
forward, ONE call of air_embed_collect: the chunk's ground-truth digits are matched to the objects the model inferred
(fp64, the reference's order of operations) and the latent and window of every matched object are copied from the model's
own buffers (``att``, ``ml``, ``vrec``, ``run_digits``, where the forward left them) to the next free rows of four
dataset-level arrays.  The row cursor and the three totals the reference prints live on the device; the chunks are
stream-ordered and the host reads four integers once, after the last one.  Reconstructions and unmatched windows never
leave the device.

``sprite_sheet(windows)`` is create_mnist_sprites (:117-131) including matplotlib's ``imsave(cmap='gray')``: the grey levels
of the sheet as a uint8 device tensor (air_embed_sprites).

``write_projector(folder, result)`` writes what TensorBoard's embedding projector opens: metadata, sprite PNG, a checkpoint
with the latents as variable ``air_mnist``, an event file and ``projector_config.pbtxt``.

Eager only: like air.vae and air.cnn the functions refuse to run while the current stream is capturing (DESIGN.md section
18.5).  There is no CPU fallback."""
import ctypes as C
import os

import numpy as np
import torch

from . import _hip as H

METADATA_FILE = "mnist_metadata.tsv"
SPRITES_FILE = "mnist_sprites.png"
CHECKPOINT_NAME = "embeddings"


class Embeddings:
    """latents [M, Z] float32, windows [M, w, w] float32, labels / ids [M] int32 of the matched digits, in (image, digit)
    order; present / inferred / matched: the totals embeddings.py:190-192 prints; sprites: the uint8 sheet, once made"""

    def __init__(self, latents, windows, labels, ids, present, inferred, matched, sprites=None):
        self.latents, self.windows, self.labels, self.ids = latents, windows, labels, ids
        self.present, self.inferred, self.matched = int(present), int(inferred), int(matched)
        self.sprites = sprites


def collect(model, images, digits, indices, positions, boxes, labels, max_distance=0.2):
    """The six lists of multi_mnist.read_test_data -> Embeddings.  `model`: an inference AIRModel (train=False)."""
    from multi_mnist import padded
    if getattr(model, "train", True):
        raise ValueError("embeddings.collect: the model must be built with train=False")
    dev = model.input_images.device
    H.require_device(model.input_images, "the model's input buffer", "embeddings.collect", capture_too=True)
    if not max_distance > 0:
        raise ValueError("embeddings.collect: max_distance must be positive")
    n, B, T = len(images), model.batch_size, model.max_steps
    Z, w, D = model.vae_latent_dimensions, model.windows_size, model.canvas_size ** 2
    if n < 1:
        raise ValueError("embeddings.collect: no images")
    counts = np.asarray(digits, np.int32).reshape(n)
    G = max(1, int(counts.max()))
    rc = H.lib().air_embed_collect_workspace_ints(T, B, B, G)
    if rc < 0:
        raise NotImplementedError("embeddings.collect: %d steps, %d digits in one image: the kernel holds %d and %d"
                                  % (T, G, H.EMBED_MAX_STEPS, H.EMBED_MAX_DIGITS))
    chunks = -(-n // B)
    rows = chunks * B                              # the last chunk is padded with blank canvases without ground truth

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    flat = np.zeros((rows, D), np.float32)
    for i, img in enumerate(images):
        flat[i] = np.asarray(img, np.float32).reshape(-1)
    gt_count = np.zeros(rows, np.int32)
    gt_count[:n] = counts
    gt = [up(a) for a in (gt_count, padded(positions, gt_count, 2, G), padded(boxes, gt_count, 2, G),
                          padded(labels, gt_count, 1, G), padded(indices, gt_count, 1, G))]
    canvases = up(flat)                            # uploaded once, like the ground truth

    capacity = max(1, int(counts.sum()))           # every ground-truth digit matched: the rows cannot run out
    out_latents = torch.empty(capacity, Z, dtype=torch.float32, device=dev)
    out_windows = torch.empty(capacity, w * w, dtype=torch.float32, device=dev)
    out_labels = torch.empty(capacity, dtype=torch.int32, device=dev)
    out_ids = torch.empty(capacity, dtype=torch.int32, device=dev)
    counters = torch.zeros(H.EMBED_COUNTERS, dtype=torch.int32, device=dev)
    match = torch.empty(B, G, dtype=torch.int32, device=dev)
    workspace = torch.empty(int(rc), dtype=torch.int32, device=dev)
    for c in range(chunks):
        lo, k = c * B, min(B, n - c * B)
        model.input_images.copy_(canvases[lo:lo + B])
        model.forward()
        a = H.EmbedCollect(H.ptr(model.att), H.ptr(model.run_digits), H.ptr(model.ml), H.ptr(model.vrec),
                           *(H.ptr(t[lo:lo + k]) for t in gt), H.ptr(match), H.ptr(counters),
                           H.ptr(out_latents), H.ptr(out_windows), H.ptr(out_labels), H.ptr(out_ids),
                           T, B, k, G, Z, w, capacity, model.canvas_size, float(max_distance))
        H.launch("air_embed_collect", dev, C.byref(a), H.ptr(workspace))
    total = counters.cpu().tolist()                # the one read-back
    if total[H.EMBED_OVERFLOW]:
        raise H.AirHipError("embeddings.collect: %d matched digits do not fit %d rows" % (total[H.EMBED_MATCHED], capacity))
    M = total[H.EMBED_MATCHED]
    return Embeddings(out_latents[:M], out_windows[:M].view(M, w, w), out_labels[:M], out_ids[:M],
                      total[H.EMBED_PRESENT], total[H.EMBED_INFERRED], M)


def sprite_sheet(windows):
    """windows [M, w, w] (or [M, w * w]) float32 on the device -> uint8 [dim * w, dim * w], dim = ceil(sqrt(M))"""
    H.require_device(windows, "windows", "embeddings.sprite_sheet", capture_too=True)
    if windows.dim() not in (2, 3) or windows.dtype != torch.float32:
        raise ValueError("embeddings.sprite_sheet: windows must be float32 [M, w, w] or [M, w * w]")
    M = int(windows.shape[0])
    w = int(windows.shape[1]) if windows.dim() == 3 else int(round(float(windows.shape[1]) ** 0.5))
    if M < 1 or w < 1 or windows.numel() != M * w * w:
        raise ValueError("embeddings.sprite_sheet: needs at least one square window (an empty sheet cannot be saved)")
    n = H.lib().air_embed_sprites_workspace_doubles(M, w)
    if n < 0:
        raise NotImplementedError("embeddings.sprite_sheet: %d windows of %d x %d are beyond the kernel's limits" % (M, w, w))
    dev, x = windows.device, windows.contiguous()
    side = H.lib().air_embed_sprite_dim(M) * w
    plane = torch.empty(side, side, dtype=torch.uint8, device=dev)
    workspace = torch.empty(int(n), dtype=torch.float64, device=dev)
    H.launch("air_embed_sprites", dev, H.ptr(x), M, w, H.ptr(workspace), H.ptr(plane))
    return plane


def probe(result, k=5, classes=10, au_threshold=0.01):
    """What the projector shows, as numbers: the leave-one-out k-nearest-neighbour accuracy of result.labels over
    result.latents, its confusion matrix and the active units (one air_latent_probe call: air.metrics has the dict's keys).
    result: an Embeddings with at least one row, on the device."""
    from .metrics import _ProbeBuffers
    latents, labels = result.latents, result.labels
    H.require_device(latents, "latents", "embeddings.probe", capture_too=True)
    H.require_device(labels, "labels", "embeddings.probe")
    if latents.dim() != 2 or latents.dtype != torch.float32 or labels.dtype != torch.int32 or labels.dim() != 1 \
            or labels.shape[0] != latents.shape[0] or labels.device != latents.device:
        raise ValueError("embeddings.probe: latents must be float32 [M, Z] and labels int32 [M] on one device")
    M, Z = int(latents.shape[0]), int(latents.shape[1])
    if M < 1:
        raise ValueError("embeddings.probe: no matched digits, nothing to probe")
    buffers = _ProbeBuffers("embeddings.probe", latents.device, M, Z, k, classes, au_threshold, False).allocate()
    buffers.run(latents.contiguous(), labels.contiguous())
    return buffers.summary()


def write_probe(folder, summary, name="latent_probe.json"):
    """probe()'s dict as JSON beside the projector files; returns the path"""
    import json
    nan = lambda v: None if v != v else v                                       # noqa: E731
    row = {key: (nan(v) if isinstance(v, float) else v) for key, v in summary.items() if not isinstance(v, np.ndarray)}
    row["confusion"] = summary["confusion"].tolist()
    for key in ("recall", "mean", "variance"):
        row[key] = [nan(float(v)) for v in summary[key]]
    path = os.path.join(os.path.abspath(folder), name)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(row, f, indent=1)
        f.write("\n")
    return path


def cluster(latents, labels=None, clusters=10, classes=10, restarts=8, max_iters=50, seed=0):
    """Do classes emerge in the latents on their own?  Exact k-means over latents [M, Z] (float32, on the device) and, where
    labels [M] (int32) are given, every cluster mapped to its majority class: one air_latent_kmeans call
    (air.metrics.LatentClusters has the dict's keys: accuracy, ari, nmi, inertia, the table, sizes, majority, centroids,
    assignment, every restart's inertia and iterations).  labels=None clusters without scoring."""
    from .metrics import _KMeansBuffers
    H.require_device(latents, "latents", "embeddings.cluster", capture_too=True)
    if labels is not None:
        H.require_device(labels, "labels", "embeddings.cluster")
        if labels.dtype != torch.int32 or labels.dim() != 1 or labels.shape[0] != latents.shape[0] or labels.device != latents.device:
            raise ValueError("embeddings.cluster: labels must be int32 [M] on the device of the latents")
        labels = labels.contiguous()
    if latents.dim() != 2 or latents.dtype != torch.float32:
        raise ValueError("embeddings.cluster: latents must be float32 [M, Z]")
    M, Z = int(latents.shape[0]), int(latents.shape[1])
    if M < 1:
        raise ValueError("embeddings.cluster: no rows, nothing to cluster")
    buffers = _KMeansBuffers("embeddings.cluster", latents.device, M, Z, clusters, classes, restarts, max_iters, seed, False).allocate()
    buffers.run(latents.contiguous(), labels)
    return buffers.summary()


def centroid_windows(model, centroids):
    """What does each discovered class look like?  centroids [n, Z] (what-codes: cluster()'s, NaN rows left out by the
    caller) -> float32 [n, w, w] on the device: the decoder's window of each, through AIRModel.decode -- centroid i is
    object 0 of its own scene with z_pres 1, the other objects absent, batch_size scenes a call.  Eager only."""
    B, N, Z, w = int(model.batch_size), int(model.max_steps), int(model.vae_latent_dimensions), int(model.windows_size)
    dev = model.input_images.device
    H.require_device(model.input_images, "the model's input buffer", "embeddings.centroid_windows", capture_too=True)
    codes = torch.as_tensor(np.asarray(_host(centroids), np.float32)).to(dev)
    if codes.dim() != 2 or int(codes.shape[1]) != Z or not bool(torch.isfinite(codes).all()):
        raise ValueError("embeddings.centroid_windows: centroids must be finite [n, %d]" % Z)
    n = int(codes.shape[0])
    out = torch.empty(n, w, w, dtype=torch.float32, device=dev)
    scales, shifts = torch.ones(B, N, 1, device=dev), torch.zeros(B, N, 2, device=dev)
    z_pres = torch.zeros(B, N, device=dev)
    z_pres[:, 0] = 1.0
    for lo in range(0, n, B):
        take = min(B, n - lo)
        latents = torch.zeros(B, N, Z, device=dev)
        latents[:take, 0] = codes[lo:lo + take]
        scenes = model.decode(latents, scales, shifts, z_pres)
        out[lo:lo + take] = scenes.windows[:take, 0].reshape(take, w, w)
    return out


def write_clusters(folder, summary, model=None, name="clusters.npz", sheet_name="cluster_sprites.png"):
    """cluster()'s dict as clusters.npz (centroids, assignment, table, sizes, majority, the restarts' inertia and iterations,
    `values` in `names` order) and, with a model, cluster_sprites.png: centroid_windows() of the clusters with members, laid
    out by sprite_sheet(); returns the paths"""
    import tf_events
    from .metrics import CLUSTER_NAMES
    folder = os.path.abspath(folder)
    os.makedirs(folder, exist_ok=True)
    paths = {"clusters": os.path.join(folder, name)}
    live = np.nonzero(summary["sizes"] > 0)[0]
    np.savez(paths["clusters"], centroids=summary["centroids"], assignment=summary["assignment"], table=summary["table"],
             sizes=summary["sizes"], majority=summary["majority"], restart_inertia=summary["restart_inertia"],
             restart_iters=summary["restart_iters"], live=live, names=np.asarray(CLUSTER_NAMES),
             values=np.asarray([summary[k] for k in CLUSTER_NAMES], np.float64),
             best=summary["best"], iters=summary["iters"], converged=summary["converged"])
    if model is not None and len(live):
        sheet = sprite_sheet(centroid_windows(model, summary["centroids"][live]))
        paths["sprites"] = os.path.join(folder, sheet_name)
        with open(paths["sprites"], "wb") as f:
            f.write(tf_events.encode_png(_host(sheet)))
    return paths


def _host(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def projector_config(folder, name="air_mnist", window_size=28):
    """the text ProjectorConfig prints for embeddings.py:207-214 (absolute paths, as the reference builds them)"""
    folder = os.path.abspath(folder)
    return ('embeddings {\n  tensor_name: "%s:0"\n  metadata_path: "%s"\n  sprite {\n    image_path: "%s"\n'
            '    single_image_dim: %d\n    single_image_dim: %d\n  }\n}\n'
            % (name, os.path.join(folder, METADATA_FILE), os.path.join(folder, SPRITES_FILE), window_size, window_size))


def write_projector(folder, result, name="air_mnist"):
    """Writes the files of embeddings.py:134-142, 201-222 into `folder`; returns their paths.  result.sprites is used when
    set, otherwise the sheet is made on the device from result.windows."""
    import tf_checkpoint
    import tf_events
    folder = os.path.abspath(folder)
    os.makedirs(folder, exist_ok=True)
    sheet = result.sprites if result.sprites is not None else sprite_sheet(result.windows)
    result.sprites = sheet
    latents = np.ascontiguousarray(_host(result.latents), dtype=np.float32)
    paths = {k: os.path.join(folder, v) for k, v in (("metadata", METADATA_FILE), ("sprites", SPRITES_FILE),
                                                     ("checkpoint", CHECKPOINT_NAME), ("state", "checkpoint"),
                                                     ("config", "projector_config.pbtxt"))}
    with open(paths["metadata"], "w") as f:
        f.write("Index\tLabel\n")
        for i, label in enumerate(_host(result.labels).tolist()):
            f.write("%d\t%d\n" % (i, label))
    with open(paths["sprites"], "wb") as f:
        f.write(tf_events.encode_png(_host(sheet)))
    tf_checkpoint.save_checkpoint(paths["checkpoint"], {name: latents})
    with open(paths["state"], "w") as f:
        f.write('model_checkpoint_path: "%s"\nall_model_checkpoint_paths: "%s"\n' % (paths["checkpoint"], paths["checkpoint"]))
    writer = tf_events.EventFileWriter(folder)     # tf.summary.FileWriter(RESULTS_FOLDER): the version record alone
    writer.close()
    paths["events"] = writer.path
    with open(paths["config"], "w") as f:
        f.write(projector_config(folder, name, int(result.windows.shape[-1])))
    return paths
