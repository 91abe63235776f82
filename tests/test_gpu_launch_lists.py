"""The launch lists AIRModel builds, pinned as data: tests/golden/launch_lists.json, written by
tests/golden/make_launch_lists.py at commit dd6808c.  Every model of the generator is rebuilt (constructed only: none of
its kernels is launched) and its forward / prologue / backward / train-step / generation lists -- (name, kernel, bytes,
flops) per launch -- and weight-gradient problems -- (M, N, K, lda) -- must equal the fixture.  A host-side change that
means to leave the launches alone proves it here; one that means to change them regenerates the fixture and says so.
"""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_launch_lists", os.path.join(GOLDEN, "make_launch_lists.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
PINNED = json.load(open(os.path.join(GOLDEN, "launch_lists.json")))


def test_the_fixture_covers_the_generators_models():
    assert sorted(PINNED) == sorted(gen.MODELS)


@pytest.mark.parametrize("name", sorted(gen.MODELS))
def test_launch_lists_equal_the_pinned_ones(name):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model as am
    batch, kw = gen.MODELS[name]
    got = json.loads(json.dumps(gen.describe(am, batch, kw)))        # (tuples -> lists, as the fixture holds them)
    want = PINNED[name]
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)
