"""The layout and the initial values of the variables, pinned as data: tests/golden/store_layout.json, written by
tests/golden/make_store_layout.py at commit 8fb0ae4.  Every store of the generator and its VAE module are rebuilt on the
CPU (the built library, no GPU) and must equal the fixture: the order of VariableStore.offsets, the panel table, name /
shape / storage offset / stride of every TF-named view, the parameter order of air.vae.VAE, and the SHA-256 of the freshly
initialised values (the Xavier draw is one numpy stream in mapping order, so an ordering mistake changes the bits).
"""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_store_layout", os.path.join(GOLDEN, "make_store_layout.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
PINNED = json.load(open(os.path.join(GOLDEN, "store_layout.json")))


@pytest.fixture(scope="module")
def rebuilt():
    return json.loads(json.dumps(gen.collect()))         # (tuples -> lists, as the fixture holds them)


def test_the_fixture_covers_the_generators_shapes():
    assert sorted(PINNED) == sorted(list(gen.STORES) + ["vae_module"])


@pytest.mark.parametrize("name", sorted(gen.STORES) + ["vae_module"])
def test_layout_equals_the_pinned_one(rebuilt, name):
    got, want = rebuilt[name], PINNED[name]
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], (name, key)
