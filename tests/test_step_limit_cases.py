"""CPU checks of the inputs of tests/test_gpu_step_limits.py (tests/step_limit_cases.py): every condition that keeps a
comparison away from a discontinuity of the step logic is asserted HERE, from the fp64 reference alone -- conditions on the
inputs, not filters on the results -- and the constructor's LDS arithmetic is checked against the figures of the kernels."""
import numpy as np
import pytest

import step_limit_cases as slc
from air import _hip as H


@pytest.mark.parametrize("train", [0, 1])
@pytest.mark.parametrize("C,w,heads", slc.ATTEND_CASES)
def test_attend_inputs_keep_items_alive_and_away_from_the_edges(C, w, heads, train):
    case, ref = slc.attend_case_and_reference(C, w, heads, train)
    m = slc.attend_margins(case, ref)
    print(m)
    assert m["S"] >= slc.S_MARGIN
    if not train:
        assert m["round"] >= slc.ROUND_MARGIN
    assert m["tap"] >= slc.TAP_MARGIN
    assert slc.SCALE_RANGE[0] <= m["scale_min"] and m["scale_max"] <= slc.SCALE_RANGE[1]
    assert m["overhang"] >= 16                     # glimpses that hang over the canvas edge: the clipped taps are read
    # the stop plan is what the reference computes: one image alive through all 16 steps, the others stop at 0, 7, 15
    mask_prev, mask = slc.expected_masks(case["stops"])
    assert np.array_equal(ref["att"][..., H.ATT_MASK], mask) and np.array_equal(ref["att"][..., H.ATT_MASK_PREV], mask_prev)
    assert case["stops"] == (None, 0, 7, 15)
    assert mask[:, 0].all() and ref["S_after"][-1, 0] < 0.99 - slc.S_MARGIN
    if train:
        assert ref["S_after"][14, 3] > 0.05        # the sum of the image that stops last is not trivial in fp32
    else:
        z = ref["att"][..., H.ATT_Z]
        assert np.isin(z, (0.0, 1.0)).all() and (ref["S_after"][mask == 1] == 0.0).all()
    assert np.isfinite(case["hid"]).all() and np.abs(case["hid"]).max() < 100.0
    assert np.isnan(case["wout"]).sum() == sum(case["wout_ld"] - wid for _, wid in slc.head_layout(*heads))


def test_padded_stride_is_the_same_case():
    case = slc.attend_case(50, 28, (1, 1, 1), 1)
    wide = slc.restride_wout(case, 64)
    assert wide["wout"].shape == (7, 64) and np.array_equal(wide["wout"][:, :1], case["wout"])
    assert np.isnan(wide["wout"][:, 1:]).all()
    a, b = slc.attend_reference(case), slc.attend_reference(wide)
    assert all(np.array_equal(a[k], b[k]) for k in ("out7", "att", "window"))


def test_bf16_rne_ties_to_even():
    x = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e-39, 0.1], np.float32)   # 1 + 2^-8: a tie; 1 + 3 * 2^-8: a tie
    got = slc.bf16_rne(x)
    assert got.tolist()[:4] == [0x3F80, 0x3F80, 0x3F82, 0xBF80]
    import torch
    assert np.array_equal(got.view(np.int16), torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy())


@pytest.mark.parametrize("C,w,Z", slc.WRITE_CASES)
def test_compose_inputs_cover_the_canvas_and_avoid_the_poles(C, w, Z):
    case, ref = slc.write_case_and_reference(C, w, Z)
    share = float(ref["in_band"].mean())
    print("share of pixels within %g of 0 or 1: %.4f; tap margin %.2e; R max %.2f; clipped share %.3f"
          % (slc.BAND, share, ref["tap"], ref["R"].max(), float((ref["R"] > 1).mean())))
    assert share <= 0.01
    assert ref["tap"] >= slc.WRITE_TAP_MARGIN
    assert (ref["R"] > 1.0).mean() >= 0.02 and ((ref["R"] > slc.BAND) & (ref["R"] < 1 - slc.BAND)).mean() >= 0.3
    assert case["images"].max() == 1.0 and (case["images"] > 0).mean() >= 0.2          # canvases with ink
    x, R = case["images"], ref["R"]
    assert not x[R < slc.ILL].any() and (x[R > 1 - slc.ILL] == 1.0).all()
    # active and inactive items, through the last step
    act = ref["active"]
    assert act[:, 0].all() and act[:7, 1].all() and not act[7:, 1].any() and act[:15, 2].all() and not act[15, 2]
    assert ref["run_digits"].tolist() == [16, 7, 15]


def test_constructor_lds_arithmetic():
    from air import air_model as am
    need = dict(am.step_lds_bytes(16, 50, 28, 64, 64, 64, 64, (2, 0)))
    # the figures of the kernels' own *_smem functions at the default shapes, worked out by hand from the layouts
    assert need["air_write_fwd"] == (16 + 112 + 16 * (400 + 784)) * 4
    assert need["air_render"] == (32 + 16 * (400 + 784)) * 4
    assert need["air_attend_fwd"] == (16 + 16 + 224 + 4 + 320 + 7 * 64 + 16 * 320 + 2500) * 4
    assert need["air_attend_bwd"] == (24 + 224 + 28 + 4 + 2500) * 4
    assert need["air_write_bwd (literal 0)"] == (64 + 400 + 50 + 224 + 784 + 1400 + 2500) * 4
    assert need["air_write_bwd (literal 2)"] == (136 + 400 + 52 + 400 + 224 + 784 + 5 * 2500) * 4
    # 160 KB is reached by compose at max_steps = 16, windows_size = 32 from canvas_size = 192 on
    am.check_step_lds(16, 191, 32, 64, 64, 64, 64)
    with pytest.raises(NotImplementedError, match="canvas_size.*max_steps"):
        am.check_step_lds(16, 192, 32, 64, 64, 64, 64)
    am.check_step_lds(3, 200, 32, 64, 64, 64, 64)
    with pytest.raises(NotImplementedError, match="air_write_bwd"):
        am.check_step_lds(3, 200, 32, 64, 64, 64, 64, (2,))
    # the query itself: the same figure serves literals 2 and 4; a null `out`, a non-positive size and a row stride of wout
    # below a head width are AIR_EINVAL
    assert dict(am.step_lds_bytes(16, 50, 28, 64, 64, 64, 64, (4,)))["air_write_bwd (literal 4)"] == need["air_write_bwd (literal 2)"]
    import ctypes as C
    lib, out, good = H.lib(), H.StepLds(), (16, 50, 28, 64, 64, 64, 64)
    assert lib.air_step_lds(*good, C.byref(out)) == 0 and out.limit == 160 * 1024
    assert lib.air_step_lds(*good, None) == -1
    for i in range(7):
        for bad in (0, -1):
            assert lib.air_step_lds(*(good[:i] + (bad,) + good[i + 1:]), C.byref(out)) == -1, (i, bad)
    assert lib.air_step_lds(16, 50, 28, 64, 65, 64, 64, C.byref(out)) == -1
