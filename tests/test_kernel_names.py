"""The kernel names the host side reports are names of kernels the built library contains.

AIRModel attaches a kernel name to every launch (air_model.KERNEL_NAMES for the entry points of _call, air_gemm_kernel_name
and its kin for the rest); bench.py groups its per-kernel times by them, tests/golden/launch_lists.json and step_plans.json
pin them, gemm_edge_kernel_names.json is keyed by them.  Nothing else ties these strings to libair_hip.so: this does, by
the library's symbol table -- the host-side launch stub of every __global__, demangled by `nm -C`.  Symbol names only."""
import itertools
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
STUB = "__device_stub__"


def _kernel_of(symbol):
    """'void (anonymous namespace)::__device_stub__k<1, 2>(T, U)' -> 'k<1, 2>': without the return type, the namespace,
    the stub prefix and the parameter list (the first parenthesis outside the template arguments)"""
    s = symbol.replace("(anonymous namespace)::", "").replace(STUB, "")
    if s.startswith("void "):
        s = s[len("void "):]
    depth = 0
    for i, ch in enumerate(s):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            return s[:i]
    return s


@pytest.fixture(scope="module")
def kernels():
    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("no nm on this machine")
    from air import _hip as H
    out = subprocess.check_output([nm, "-C", H.LIB_PATH], text=True)
    names = {_kernel_of(line.split(" ", 2)[2]) for line in out.splitlines() if STUB in line}
    assert len(names) > 100, len(names)              # (213 when this was written: the parser found the stubs)
    return names


def _pinned(x, out):
    """kernel strings of a fixture: the second field of every [name, kernel, ...] launch, and the captured x.Wx lists"""
    if isinstance(x, dict):
        for k, v in x.items():
            if k == "xwx":
                out.update(v)
            else:
                _pinned(v, out)
    elif isinstance(x, list):
        if len(x) >= 2 and isinstance(x[0], str) and isinstance(x[1], str) and (len(x) == 2 or isinstance(x[2], int)):
            out.add(x[1])
        for v in x:
            _pinned(v, out)
    return out


@pytest.mark.parametrize("fixture", ["launch_lists.json", "step_plans.json"])
def test_pinned_launch_kernels_exist(kernels, fixture):
    with open(os.path.join(GOLDEN, fixture)) as f:
        names = _pinned(json.load(f), set())
    assert len(names) >= 20, names
    assert sorted(names - kernels) == []


def test_gemm_edge_kernel_names_exist(kernels):
    with open(os.path.join(GOLDEN, "gemm_edge_kernel_names.json")) as f:
        names = set(json.load(f))
    assert len(names) >= 100
    assert sorted(names - kernels) == []


def test_entry_point_table_names_kernels(kernels):
    """every fixed value of air_model.KERNEL_NAMES, and every template over the values AIRModel._call fills in"""
    from air import air_model as am
    domain = dict(slabs=(0, 4), twins=("true", "false"), bf16=("", "_bf16"), filters=range(1, 9), gauss=("", "_gauss"))
    keys = sorted(domain)
    for entry, name in am.KERNEL_NAMES.items():
        assert hasattr(am.H.lib(), entry), entry
        if name is None:                              # (the library names the kernel of the descriptor itself)
            continue
        if "{" not in name:
            assert name in kernels, (entry, name)
            continue
        for values in itertools.product(*(domain[k] for k in keys)):
            filled = name.format(**dict(zip(keys, values)))
            assert filled in kernels, (entry, filled)
    assert am.KERNEL_NAMES["air_colsum"] == "colsum_kernel"
