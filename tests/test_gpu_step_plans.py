"""What AIRModel's runners and its capture enqueue, pinned as data: tests/golden/step_plans.json, written by
tests/golden/make_step_plans.py at commit 281a936.  Every model of the generator is rebuilt, every flow repeated (an eager
train step, with and without injected noise; _run_forward + _run_backward; a captured 3-step replay with and without a
between_steps hook; an uncaptured forward of a test model) and the launches that reached the stream -- (name, kernel), in
order -- must equal the fixture.  A second test reads the fixture alone: every branch the runners have is taken in it.
A third compares what capture_graph records with what it enqueued under capture.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_step_plans", os.path.join(GOLDEN, "make_step_plans.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
PINNED = json.load(open(os.path.join(GOLDEN, "step_plans.json")))

TRAIN = sorted(n for n, kw in gen.MODELS.items() if kw["train"])
EAGER = ("train_step_ops", "eager", "run", "eager_injected", "run_injected")


@pytest.mark.parametrize("name", sorted(gen.MODELS))
def test_step_plans_equal_the_pinned_ones(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model as am
    got = json.loads(json.dumps(gen.describe(am, gen.MODELS[name])))
    want = PINNED[name]
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)


@pytest.mark.parametrize("injected", [False, True])
def test_the_capture_records_what_it_enqueued(injected):
    """captured_step_ops() is the plan that went to the stream under capture, launch for launch -- with injected noise
    that includes the schedules-only prologue launch in front of x.Wx (not part of the fixture: the record of the code the
    fixture was written with left that launch out)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model as am
    from oracle.synth import blob_canvases
    images, targets = blob_canvases(gen.BATCH, gen.CANVAS, 2, seed=3)
    am.reset_default_graph()
    m = am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, **gen.MODELS["bf16"])
    if injected:
        m.set_noise(gen._no_noise({}))
    calls = gen.recorded(am, lambda: m.capture_graph(steps=2))
    steps = [gen._ops(m.captured_step_ops(i)) for i in (0, 1)]
    assert calls[-len(steps[0]) - len(steps[1]):] == steps[0] + steps[1]       # (in front of them: the warm-up)
    for step, xwx in zip(steps, m.captured_xwx_ops()):
        assert ("air_step_begin" in _names(step)) == injected
        assert step[int(injected)] == [xwx.name, xwx.kernel] and _names(step)[0] == ("air_step_begin" if injected else xwx.name)
    am.reset_default_graph()


def _names(ops):
    return [n for n, _ in ops]


def _kernels(ops):
    return [k for _, k in ops]


def _flows(model):
    """(flow name, [name, kernel] list) of every list the fixture holds for one model, captured steps one by one"""
    for key, val in sorted(PINNED[model].items()):
        if isinstance(val, dict):
            for i, step in enumerate(val["steps"]):
                yield "%s[%d]" % (key, i), step
        else:
            yield key, val


def test_the_fixture_takes_every_branch():
    assert sorted(PINNED) == sorted(gen.MODELS)
    for model in TRAIN:
        assert sorted(PINNED[model]) == sorted(EAGER + ("captured", "captured_hook"))
        for cap in ("captured", "captured_hook"):
            assert len(PINNED[model][cap]["steps"]) == 3 and len(PINNED[model][cap]["xwx"]) == 3
    assert sorted(PINNED["bf16_test"]) == ["forward", "forward_injected"]

    # compose inside the write-backward launch: every captured step of bf16, none without the fold or in the exact order
    def folded(model):
        return [any("compose_write_bwd" in k for k in _kernels(ops)) for flow, ops in _flows(model) if flow.startswith("captured")]
    assert folded("bf16") == [True] * 6
    assert folded("bf16_no_fold") == [False] * 6 and folded("bf16_exact") == [False] * 6
    # ... and an eager step never has it
    for model in TRAIN:
        for key in EAGER:
            assert not any("compose_write_bwd" in k for k in _kernels(PINNED[model][key])), (model, key)

    # the twin-operand x.Wx opens steps 1 and 2 of the replay, not step 0, not with a hook, not where x.Wx carries the prologue
    def opens_with_twin(model, cap):
        return [_names(step)[0].startswith("xWx16+lstm0") for step in PINNED[model][cap]["steps"]]
    assert opens_with_twin("bf16", "captured") == [False, True, True]
    assert opens_with_twin("bf16", "captured_hook") == [False] * 3
    assert opens_with_twin("bf16_n1", "captured") == [False] * 3
    for model in ("bf16", "bf16_n1"):
        for flow, ops in _flows(model):
            if (model, flow) not in (("bf16", "captured[1]"), ("bf16", "captured[2]")):
                assert not any(n.startswith("xWx16+lstm0") for n in _names(ops)), (model, flow)
    # (the recorded x.Wx kernel names are those of the steps' first launches)
    for model in TRAIN:
        if model != "bf16_cnn":
            for cap in ("captured", "captured_hook"):
                assert PINNED[model][cap]["xwx"] == [_kernels(step)[0] for step in PINNED[model][cap]["steps"]], (model, cap)

    # the conv front-end is first in every flow of its model and in no flow of another
    for flow, ops in _flows("bf16_cnn"):
        assert _names(ops)[0] == "cnn_fwd", flow
    for model in sorted(gen.MODELS):
        if model != "bf16_cnn":
            assert not any("cnn_fwd" in _names(ops) for flow, ops in _flows(model)), model

    # the schedules-only prologue launch: the injected-noise flows and no other
    for model in sorted(gen.MODELS):
        for flow, ops in _flows(model):
            assert ("air_step_begin" in _names(ops)) == flow.endswith("_injected"), (model, flow)

    # the batch means' own launch closes an uncaptured forward; a train step has none (they ride in the write backward)
    for flow in ("forward", "forward_injected"):
        assert _kernels(PINNED["bf16_test"][flow])[-1] == "finalize_kernel"
    for model in TRAIN:
        for flow, ops in _flows(model):
            if not flow.startswith("run"):               # (_run_forward(s) alone is a forward: it finalizes)
                assert "finalize_kernel" not in _kernels(ops), (model, flow)
