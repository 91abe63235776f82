"""The twin tiles of air_wgrad_grouped after their chain was shortened: a one-round path of its own,
bias sums whose loads leave early in the tiles that own a column, square sums parked per tile and published behind the last
store.  (The interior form of the twin staging that the shapes below were also chosen for was measured and removed; the
shapes stay: interior and edge tiles of both piece widths in one launch.)

Every case is one precision-1 launch with twins, compared BIT FOR BIT -- dW, db, every partial, the step word -- with the launch
of the same descriptors without twins (A16 = dY16 = NULL: tile_bf16, which DESIGN.md section 28 defines as bit-identical).
Both run on the poisoned buffers of tests/test_gpu_wgrad_edges.py: NaN pads, dW between guard rows, db and the partials between
sentinel guards, all checked; the values are checked against float64 with that test's bounds on the way.

Shapes are the smallest that take each branch (BT = 64, one round = 192 rows):
  (132, 128, 192)  two full block-rows and a ragged one of 4 rows, with lda = 132 (8-byte rows) and lda = 136 (16-byte rows).
                   With db: block-row 0 owns the bias columns (whole images, sent early), block-rows 1 and 2 do not.
  (132, 136, 192)  the last column tile (8 columns) is an edge tile of dY; its bias column is ragged
  (64, 128, 192) + (64, 64, 64), both with db, in one launch: three images / one image per owner
  (132, 256, 64)   with and without db, `strip` as fill_table picks it; tile partials index by index
  (196, 8192, 64)  512 tiles: strips of 2 whose A block has 8-byte rows -- three block-rows inside M, a ragged one; bias owners
                   nt % 4; every tile's partial parked and published behind the strip
  (68, 72, 72)     K is no whole number of images: the owner's sums stay behind the MFMAs (bias_tw)
and two launches in a row on one istate count 2 steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import wgrad_edge_cases as wec
from test_gpu_gemm_edges import DEV
from test_gpu_wgrad_edges import _operands, _run_launch, _stream, _vec, _OutW

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _tw(M, N, K, pads, **kw):
    c = wec._case("chain", 1, M, N, K, pads, "", twins=True, **kw)
    c["path"], c["bias"] = wec.path_of(c), wec.bias_of(c)
    return c


LAUNCHES = {
    "masked-lda132": [_tw(132, 128, 192, (0, 0, 0))],
    "interior-lda136": [_tw(132, 128, 192, (4, 0, 0))],
    "interior-lda136-no-db": [_tw(132, 128, 192, (4, 0, 0), db=False)],
    "edge-column-N136": [_tw(132, 136, 192, (4, 0, 0))],
    "owners-3-images-and-1": [_tw(64, 128, 192, (0, 0, 0)), _tw(64, 64, 64, (0, 0, 0))],
    "K64-two-of-a-row": [_tw(132, 256, 64, (4, 0, 0))],
    "K64-two-of-a-row-no-db": [_tw(132, 256, 64, (4, 0, 0), db=False)],
    "strips-A8-inside-and-ragged": [_tw(196, 8192, 64, (0, 0, 0))],
    "K72-late-bias": [_tw(68, 72, 72, (8, 8, 4))],
}


def test_the_cases_take_the_paths_they_are_written_for():
    kinds = {k: [c["path"]["kind"] for c in v] for k, v in LAUNCHES.items()}
    assert kinds.pop("strips-A8-inside-and-ragged") == ["strip"]
    assert all(k == "tile_bf16_tw" for v in kinds.values() for k in v)
    s = LAUNCHES["strips-A8-inside-and-ragged"][0]
    assert s["path"] == dict(kind="strip", G=2, A8=True, xcd_map=False) and wec.bias_mod(s) == 4
    assert wec.twin_pieces(LAUNCHES["masked-lda132"][0])[0] == 8 and wec.rows16(0, LAUNCHES["interior-lda136"][0]["lda"])


@pytest.mark.parametrize("name", list(LAUNCHES))
def test_twin_launch_is_bit_identical_to_the_fp32_operand_launch(H, name):
    bad, forms = _run_launch(H, wec.launch(name, LAUNCHES[name]), np.random.RandomState(9000 + len(name)), "chain")
    assert len(forms) == 2                                   # the twin launch and the one without twins
    assert not bad, "%d failures:\n%s" % (len(bad), "\n".join(bad[:40]))


def test_two_launches_in_a_row_count_two_steps(H):
    cases = LAUNCHES["interior-lda136"] + LAUNCHES["owners-3-images-and-1"]
    rng = np.random.RandomState(9100)
    ops = [_operands(c, rng) for c in cases]
    ist = torch.zeros(8, dtype=torch.int32, device=DEV)
    runs = []
    for twins in (True, True, False):
        cs = [c if twins else wec.without_twins(c) for c in cases]
        dW = [_OutW(c["M"], c["N"], c["ldc"]) for c in cs]
        db = [_vec(c["N"]) for c in cs]
        probs = []
        for c, op, w, b in zip(cs, ops, dW, db):
            ptr = dict(A=op["Ain"].ptr, dY=op["Yin"].ptr, dW=w.ptr, db=b.ptr)
            if twins:
                ptr.update(A16=op["A16"].ptr, dY16=op["Y16"].ptr)
            probs.append(wec.descriptor(H, c, ptr))
        arr = (H.Wgrad * len(probs))(*probs)
        part = _vec(wec.num_partials(cs))
        if len(runs) < 2:                                    # the two twin launches share the step word
            H.check(H.lib().air_wgrad_grouped(arr, len(probs), 1, C.c_void_p(part.ptr), C.c_void_p(ist.data_ptr()), _stream()), "air_wgrad_grouped")
        else:
            H.check(H.lib().air_wgrad_grouped(arr, len(probs), 1, C.c_void_p(part.ptr), None, _stream()), "air_wgrad_grouped")
        runs.append((dW, db, part))
    torch.cuda.synchronize()
    got = ist.cpu().numpy()
    assert int(got[H.IST_GLOBAL_STEP]) == 2 and not got[1:].any(), got.tolist()
    for dW, db, part in runs[1:]:
        for a, b in zip(runs[0][0] + runs[0][1] + [runs[0][2]], dW + db + [part]):
            assert a.check()[0] == [] and b.check()[0] == []
            assert np.array_equal(a.host(), b.host())
