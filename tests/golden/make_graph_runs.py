"""Generates tests/golden/graph_runs.npz: what the reference's own serialized training graph
(its model/air-model.meta, executed node by node by oracle/graphdef_exec.py) returns for the inputs
of tests/test_graph_exec.py's forward, dynamic-batch and fp64 backward + Adam cases.  Run from the
repo root where the reference is checked out (the graph is a 3.9 MB program and is not committed):

    python tests/golden/make_graph_runs.py <reference>/model/air-model.meta

Recorded per case: the outputs the reference's callers fetch, as "dtype|shape|sha256 of the bytes"
(the tests assert bit identity, which the digest keeps), the loop trip counts and annealed prior, the
latent samples of the test model, and for the fp64 cases every gradient's norm and the fixed element
subsets of make_graph_golden.subsample_index (every STRIDE-th) of the gradient and of the ApplyAdam variable / slot updates.
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import graphdef_exec as gx  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "graph_runs.npz")
ATTRS = ("reconstruction", "reconstruction_loss", "rec_num_digits", "rec_scales", "rec_shifts", "rec_st_back",
         "rec_windows", "z_pres_probs", "z_pres_kls", "scale_kls", "shift_kls", "vae_kls", "loss", "accuracy")
TRAIN_CASES = [(0, 3, 1), (3000, 11, 7), (40000, 5, 2)]          # (global_step, seed_images, seed_noise)
TEST_CASES = [(4, 40000), (7, 0), (1, 2000)]                      # (batch, global_step)
BWD_STEPS = (0, 40000)
STRIDE = 4                                                        # every 4th element of the fixed subset: 512 per large tensor


def digest(a):
    a = np.asarray(a)
    return "%s|%s|%s" % (a.dtype.str, a.shape, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest())


def _mk():
    spec = importlib.util.spec_from_file_location("make_graph_golden", os.path.join(ROOT, "tests", "golden", "make_graph_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main(meta):
    mk = _mk()
    version, nodes = gx.load_graph(meta)
    assert version == "1.3.0" and len(nodes) == 15022
    out = {}
    for step, si, sn in TRAIN_CASES:
        images, targets, params, noise = mk.inputs(seed_images=si, seed_noise=sn)
        if step == 40000:
            noise["u"][0] = 1e-4
        ex = gx.Executor(nodes, gx.air_feeds(nodes, params, images, targets, noise, step))
        T = gx.output_tensors("air")
        vals = dict(zip(T, ex.run(list(T.values()))))
        p = "train/%d/" % step
        out[p + "z_pres_prior_log_odds"] = np.asarray(vals["z_pres_prior_log_odds"])
        out[p + "trips"] = np.int32(ex.trip_count(gx.FWD_FRAME))
        for k in ATTRS:
            out[p + k] = np.array(digest(vals[k]))
    for batch, step in TEST_CASES:
        images, targets, params, noise = mk.inputs(batch=batch)
        ex = gx.Executor(nodes, gx.test_model_feeds(params, images, targets, noise, step))
        T = gx.output_tensors("air_1")
        vals = dict(zip(T, ex.run(list(T.values()))))
        p = "test/%d_%d/" % (batch, step)
        out[p + "z_pres_prior_log_odds"] = np.asarray(vals["z_pres_prior_log_odds"])
        out[p + "trips"] = np.int32(ex.trip_count("air_1/rnn/while/air_1/rnn/while/"))
        out[p + "latent_samples"] = np.asarray(vals["_graph_latent_samples"])
        for k in ATTRS:
            out[p + k] = np.array(digest(vals[k]))
    for step in BWD_STEPS:
        images, targets, params, noise = mk.inputs()
        if step == 40000:
            noise["u"][0] = 1e-4
        f64 = np.float64
        ex = gx.Executor(nodes, gx.air_feeds(nodes, params, images, targets, noise, step, float_dtype=f64), f64)
        adam = gx.adam_nodes(nodes)
        names = list(params.keys())
        grads = dict(zip(names, ex.run([gx.raw_gradient_tensor(nodes, adam[k]) for k in names])))
        p = "bwd/%d/" % step
        out[p + "global_norm"] = np.float64(ex.run(["air/training/global_norm/global_norm"])[0])
        out[p + "z_pres_prior_log_odds"] = np.float64(ex.run(["air/z_pres_prior_log_odds_log"])[0])
        out[p + "loss"] = np.float64(ex.run(["air/summaries/loss"])[0])
        out[p + "fwd_trips"] = np.int32(ex.trip_count(gx.FWD_FRAME))
        out[p + "bwd_trips"] = np.int32(ex.trip_count(gx.BWD_FRAME))
        ex.run([adam[k].name for k in names])
        for k in names:
            g = np.asarray(grads[k], f64)
            idx = mk.subsample_index(k, g.size)[::STRIDE]
            a = ex.assigned[gx.SCOPE + k]
            out[p + "grad_norm/" + k] = np.float64(np.linalg.norm(g))
            out[p + "grad_sub/" + k] = g.reshape(-1)[idx]
            out[p + "var_sub/" + k] = np.asarray(a["var"], f64).reshape(-1)[idx]
            out[p + "m_sub/" + k] = np.asarray(a["m"], f64).reshape(-1)[idx]
            out[p + "v_sub/" + k] = np.asarray(a["v"], f64).reshape(-1)[idx]
    np.savez_compressed(OUT, **out)
    print("wrote %d arrays, %.0f KB" % (len(out), os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main(sys.argv[1])
