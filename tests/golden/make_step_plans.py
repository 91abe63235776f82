"""Generates tests/golden/step_plans.json: what AIRModel's runners and its capture ENQUEUE, as data.

    python tests/golden/make_step_plans.py [OUT.json]

launch_lists.json pins the lists the builders make (_fwd, _bwd, train_step_ops()).  This file pins what becomes of them
when a step runs: for every model of MODELS and every flow below, the launches in the order they reach the stream, each
as [name, kernel].  No pointers, bytes or flops (launch_lists.json has those).  tests/test_gpu_step_plans.py rebuilds
the models, repeats the flows and asserts equality: a change of the host code that decides which launches make up a step
proves there that it decides as before.

Eager flows are recorded by wrapping _Op.__call__ for the duration of the flow (the wrapper appends the op, then calls the
original); captured flows are read from captured_step_ops(i) and captured_xwx_kernels().  Flows of a train model, in the
order they run on ONE model (the injected ones last: injected noise stays on once set):

    train_step_ops      the list train_step_ops() returns
    eager               one training(eager=True)
    run                 _run_forward(s); _run_backward(s)
    captured            capture_graph(steps=3): {"steps": [step 0, step 1, step 2], "xwx": captured_xwx_kernels()}
    captured_hook       the same with between_steps=lambda i: None
    eager_injected      one training(eager=True) after set_noise
    run_injected        _run_forward(s); _run_backward(s) after set_noise

and of a test model: forward, forward_injected (an uncaptured forward() each).  The injected noise is "no noise": zero
normals, and u = 1/2 for the Concrete uniform (logit(1/2) = 0; u = 0 would be log(0)).  Each flow's GPU work is a handful
of B = 16 steps.

The committed fixture was written at commit 281a936, the parent of the change that added this script and made the
runners, train_step_ops() and capture_graph read one launch plan per step; the script reads only names that exist on both
sides, so it runs unchanged there and here.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tf-attend-infer-repeat_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden", "step_plans.json")
BATCH, CANVAS = 16, 50
# name -> constructor arguments; the smallest set that takes every branch of the runners and of the capture
MODELS = {
    "bf16": dict(gemm_precision="bf16", train=True),
    "bf16_no_fold": dict(gemm_precision="bf16", train=True, compose_fold=False),
    "bf16_exact": dict(gemm_precision="bf16", train=True, backward="exact"),
    "bf16_n1": dict(gemm_precision="bf16", train=True, max_steps=1, max_digits=1),   # the x.Wx launch carries the prologue
    "fp32": dict(gemm_precision="fp32", train=True),
    "bf16_cnn": dict(gemm_precision="bf16", train=True, cnn=True),
    "bf16_test": dict(gemm_precision="bf16", train=False),
}


def _ops(ops):
    return [[op.name, op.kernel] for op in ops]


def recorded(am, flow):
    """[name, kernel] of every op called while flow() runs, in call order"""
    seen, call = [], am._Op.__call__

    def wrapper(op, stream):
        seen.append(op)
        return call(op, stream)
    am._Op.__call__ = wrapper
    try:
        flow()
    finally:
        am._Op.__call__ = call
    torch.cuda.synchronize()
    return _ops(seen)


def _no_noise(kw):
    N, Z, d = kw.get("max_steps", 3), 50, 28 * 28
    z = lambda *shape: torch.zeros(*shape)
    return dict(eps_scale=z(N, BATCH, 1), eps_shift=z(N, BATCH, 2), eps_z=z(N, BATCH, Z), eps_x=z(N, BATCH, d),
                u=torch.full((N, BATCH), 0.5))


def describe(am, kw):
    """the flows of one freshly constructed model, as JSON-able data"""
    from oracle.synth import blob_canvases
    images, targets = blob_canvases(BATCH, CANVAS, 2, seed=3)
    kw = dict(kw)
    kw.setdefault("cnn", False)
    am.reset_default_graph()
    m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), scope="air", seed=0,
                    noise_seed=0, **kw)
    if not kw["train"]:
        out = {"forward": recorded(am, m.forward)}
        m.set_noise(_no_noise(kw))
        out["forward_injected"] = recorded(am, m.forward)
        am.reset_default_graph()
        return out

    def run():
        s = m._stream()
        m._run_forward(s)
        m._run_backward(s)

    def captured(**hooks):
        m.capture_graph(steps=3, **hooks)
        got = {"steps": [_ops(m.captured_step_ops(i)) for i in range(3)], "xwx": list(m.captured_xwx_kernels())}
        m.release_graph()
        torch.cuda.synchronize()
        return got

    out = {"train_step_ops": _ops(m.train_step_ops()),
           "eager": recorded(am, lambda: m.training(eager=True)),
           "run": recorded(am, run),
           "captured": captured(),
           "captured_hook": captured(between_steps=lambda i: None)}
    m.set_noise(_no_noise(kw))
    out["eager_injected"] = recorded(am, lambda: m.training(eager=True))
    out["run_injected"] = recorded(am, run)
    am.reset_default_graph()
    return out


def collect():
    from air import air_model as am
    return {name: describe(am, kw) for name, kw in MODELS.items()}


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(collect(), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)
