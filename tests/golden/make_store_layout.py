"""Generates tests/golden/store_layout.json: the layout and the initial values of the variables, as data.

    python tests/golden/make_store_layout.py [OUT.json]

Needs the built library and no GPU: every store and module is constructed on the CPU.  For every shape of STORES it records
of VariableStore(hp, cpu, seed=0) the order of `offsets`, `n`, `num_trainable`, the panel table with `panel_off` and
`wx_exclusive`, (name, shape, storage offset, stride) of every entry of `variables` in order, and the SHA-256 of `params`;
of one air.vae.VAE the parameter names in parameters() order, the variables() views and the SHA-256 of the parameter bytes.
The order of these decides checkpoints, the panel table and the Xavier draw (one numpy stream in mapping order):
tests/test_store_layout.py rebuilds them and asserts equality, so a host-side change that means to leave the layout alone
proves it there.

The committed fixture was written at commit 8fb0ae4, the parent of the change that added this script and gave the VAE's
layer chain one owner (air/_layers.py); the script reads only attributes that exist there, so it runs unchanged on both
sides.
"""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tf-attend-infer-repeat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden", "store_layout.json")
# the odd shape of tests/golden/make_launch_lists.py: D % 4 = 1, no Wx panel, one recognition and one generative layer, Z = 7
ODD = dict(max_steps=4, max_digits=3, canvas_size=33, windows_size=17, vae_latent_dimensions=7, rnn_units=80,
           vae_recognition_units=(50,), vae_generative_units=(30,), scale_hidden_units=24,
           shift_hidden_units=24, z_pres_hidden_units=40)
# name -> what DEFAULT_HP is updated with
STORES = {
    "default": {},
    "odd": ODD,
    "canvas68": dict(canvas_size=68, rnn_units=16),          # D = 4624 > 4096: the no-Wx-panel branch at a small size
}
VAE_ARGS = (36, (24, 16), 6, (16, 24))
VAE_SEED = 5


def _sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def _views(mapping):
    return [[k, [int(s) for s in v.shape], int(v.storage_offset()), [int(s) for s in v.stride()]] for k, v in mapping.items()]


def describe_store(am, vae_mod, hp):
    st = am.VariableStore(hp, torch.device("cpu"), seed=0)
    names = [k for k in st.variables if k.startswith("vae/")]
    assert names == vae_mod.VAE.variable_names(hp["vae_recognition_units"], hp["vae_generative_units"])
    return {"offsets": [[k, int(v)] for k, v in st.offsets.items()], "n": int(st.n), "num_trainable": int(st.num_trainable),
            "panels": [[int(q.src_off), int(q.dst_off), int(q.K), int(q.N), int(q.gates), int(q.exclusive)] for q in st.panels],
            "panel_off": [[k, int(v)] for k, v in st.panel_off.items()], "wx_exclusive": bool(st.wx_exclusive),
            "variables": _views(st.variables), "params_sha256": _sha([st.params])}


def describe_vae(vae_mod):
    m = vae_mod.VAE(*VAE_ARGS, device="cpu", seed=VAE_SEED)
    return {"parameters": [k for k, _ in m.named_parameters()], "variables": _views(m.variables()),
            "params_sha256": _sha(list(m.parameters()))}


def collect():
    from air import air_model as am
    from air import vae as vae_mod
    from oracle.air_oracle import DEFAULT_HP
    out = {name: describe_store(am, vae_mod, dict(DEFAULT_HP, **kw)) for name, kw in STORES.items()}
    out["vae_module"] = describe_vae(vae_mod)
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(collect(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)
