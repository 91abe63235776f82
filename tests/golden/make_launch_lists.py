"""Generates tests/golden/launch_lists.json: the launch lists AIRModel builds, as data.

    python tests/golden/make_launch_lists.py [OUT.json]

Needs a GPU only because AIRModel wants device tensors: the models are constructed, none of their kernels is launched.
For every model of MODELS it records (name, kernel, nbytes, flops) of each op of the forward list, of the op that carries
the step prologue (and its index), of the backward list, of train_step_ops() and of the two generation lists, and
(M, N, K, lda) of every weight-gradient problem.  No pointers.  tests/test_gpu_launch_lists.py rebuilds the models
and asserts equality: a change of the host code that is meant to leave the launches alone proves it there.

The committed fixture was written at commit dd6808c, the parent of the change that added this script and retired the
model's environment switches; the script reads only attributes that exist there, so it runs unchanged on both sides.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tf-attend-infer-repeat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden", "launch_lists.json")
BIG = dict(canvas_size=128, max_steps=5, max_digits=4)
# the odd shape of tests/test_gpu_configs.py (RAGGED[2]): D % 4 = 1, so neither the first-step fusion nor the Wx panel
ODD = dict(max_steps=4, max_digits=3, canvas_size=33, windows_size=17, vae_latent_dimensions=7, rnn_units=80,
           vae_recognition_units=(50,), vae_generative_units=(30,), scale_hidden_units=24,
           shift_hidden_units=24, z_pres_hidden_units=40)
# name -> (batch, constructor arguments); the smallest set that takes every branch of the builders
MODELS = {
    "bf16": (64, dict(gemm_precision="bf16", train=True)),
    "fp32": (64, dict(gemm_precision="fp32", train=True)),
    "bf16_test": (64, dict(gemm_precision="bf16", train=False)),
    "bf16_no_twins": (64, dict(gemm_precision="bf16", train=True, bf16_twins=False)),
    "bf16_carried": (64, dict(gemm_precision="bf16", train=True, backward="reference_carried")),
    "bf16_exact": (64, dict(gemm_precision="bf16", train=True, backward="exact")),
    "bf16_128": (64, dict(gemm_precision="bf16", train=True, **BIG)),        # D > 4096 tiling; N * B = 320: wb_order
    "bf16_odd": (37, dict(gemm_precision="bf16", train=True, **ODD)),
    "bf16_xw_tile": (64, dict(gemm_precision="bf16", train=True, xw_tile=(4, 2, 4))),
}


def _ops(ops):
    return [[op.name, op.kernel, int(op.nbytes), int(op.flops)] for op in ops]


def describe(am, batch, kw):
    """the launch lists of one freshly constructed model, as JSON-able data"""
    canvas = kw.get("canvas_size", 50)
    am.reset_default_graph()
    m = am.AIRModel(torch.zeros(batch, canvas * canvas, device="cuda"), torch.zeros(batch, dtype=torch.int32, device="cuda"),
                    cnn=False, scope="air", **kw)
    hi, hop = m._begin_host
    out = {"fwd": _ops(m._fwd), "begin_host": [int(hi)] + _ops([hop]), "bwd": _ops(m._bwd),
           "train_step_ops": _ops(m.train_step_ops()) if m.train else None,
           "generate": _ops(m.generate_ops(False, False, True)),
           "decode_noise": _ops(m.generate_ops(True, True, True)),
           "wgrad": [[int(q.M), int(q.N), int(q.K), int(q.lda)] for q in m._wgrad_arr] if m.train else None}
    am.reset_default_graph()
    return out


def collect():
    from air import air_model as am
    return {name: describe(am, batch, kw) for name, (batch, kw) in MODELS.items()}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(collect(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)
