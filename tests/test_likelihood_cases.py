"""CPU checks for the Gaussian pixel likelihood (AIR_LIK_GAUSSIAN): the conditions of the inputs that
tests/test_gpu_likelihood.py relies on, asserted from the fp64 reference alone (conditions on the inputs, not filters on the
results), and the argument errors the library reports on the host before any launch."""
import ctypes as C

import numpy as np
import pytest

import abi_check as abi
import likelihood_cases as lc
import step_limit_cases as slc


@pytest.fixture(scope="module")
def H():
    return abi.hip()


@pytest.mark.parametrize("Cc,w,Z", lc.COMPOSE_CASES)
def test_compose_cases_have_passing_and_clipped_pixels_away_from_the_clip_edges(Cc, w, Z):
    case, ref, g = lc.compose_case_and_reference(Cc, w, Z)
    assert (case["N"], case["B"]) == (16, 3)
    in_band, passes = ref["in_band"], g["passes"]
    cmp = ~in_band
    print("C = %d: in band %.4f %%, compared and passing %.1f %%, compared and clipped %.1f %%"
          % (Cc, 100 * in_band.mean(), 100 * (cmp & passes).mean(), 100 * (cmp & ~passes).mean()))
    assert in_band.mean() <= 0.01
    assert (cmp & passes).mean() >= 0.30
    assert (cmp & ~passes).mean() >= 0.02
    assert float(case["dyn"][lc.H.DYN_LIK_STD]) == np.float32(0.3)
    # the gradient is bounded on every canvas: |d loss / d canvas| <= gsc / sigma^2 (x and r lie in [0, 1])
    assert np.abs(g["d_recon"]).max() <= g["gsc"] / g["sigma"] ** 2
    assert (Cc * Cc <= 4096) == (Cc < 65)                     # both sides of the image-prefetch threshold are among the cases


def test_masked_image_has_a_zero_canvas_whose_tie_passes():
    case, ref, g = lc.masked_case_and_reference()
    b = lc.MASKED_IMAGE
    base, base_ref, _ = lc.compose_case_and_reference(*lc.COMPOSE_CASES[0])
    assert not ref["active"][:, b].any() and ref["run_digits"][b] == 0
    assert not ref["R"][b].any() and not ref["recon"][b].any()
    assert g["passes"][b].all()
    x = case["images"][b].astype(np.float64)
    assert x.max() > 0.0                                      # ink that no glimpse explains
    np.testing.assert_array_equal(g["d_recon"][b], -g["gsc"] * x / g["sigma"] ** 2)
    for other in (0, 2):                                      # the other images are the base case's
        assert np.array_equal(ref["R"][other], base_ref["R"][other])
    assert ref["tap"] >= slc.WRITE_TAP_MARGIN


def _write_fwd(H, **kw):
    p = abi.host_ptr
    a = H.WriteFwd(p(), p(), p(), p(), p(), p(), p(), p(), p(), p(), p(), 3, 3, 50, 28, 50, None)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _write_bwd_for(H, f):
    p = abi.host_ptr
    return H.WriteBwd(f.d_recon, f.vrec, f.att, p(), p(), f.B, f.N, f.C, f.w, 2, f.loss_item, p(), f.run_digits, p(), None, None)


def test_positional_descriptor_is_the_bernoulli_path(H):
    a = _write_fwd(H)
    assert a.likelihood == 0 == H.LIK_BERNOULLI and H.LIK_GAUSSIAN == 1
    assert H.WriteFwd._fields_[-1][0] == "likelihood"


def test_unknown_likelihood_is_refused_before_any_launch(H):
    lib = H.lib()
    for bad in (2, -1, 7):
        assert lib.air_write_fwd(C.byref(_write_fwd(H, likelihood=bad)), None) == H.EINVAL, bad
    # ... and a null argument still is, under either likelihood
    assert lib.air_write_fwd(C.byref(_write_fwd(H, likelihood=H.LIK_GAUSSIAN, images=None)), None) == H.EINVAL


def test_fold_refuses_the_gaussian_likelihood(H):
    """air_write_fwd_bwd has not been taught the likelihood: AIR_ELIMIT, `the caller keeps its two launches`, from the name
    query and from the launcher (both read one host-side plan: no GPU is touched)"""
    lib, buf = H.lib(), C.create_string_buffer(96)
    f = _write_fwd(H)
    b = _write_bwd_for(H, f)
    assert lib.air_write_fwd_bwd_kernel_name(C.byref(f), C.byref(b), buf, 96) == 0
    assert buf.value == b"compose_write_bwd_graph_kernel"
    f.likelihood = H.LIK_GAUSSIAN
    assert lib.air_write_fwd_bwd_kernel_name(C.byref(f), C.byref(b), buf, 96) == H.ELIMIT
    assert lib.air_write_fwd_bwd(C.byref(f), C.byref(b), abi.host_ptr(), None) == H.ELIMIT
    f.likelihood = 2
    assert lib.air_write_fwd_bwd_kernel_name(C.byref(f), C.byref(b), buf, 96) == H.EINVAL


def test_gauss_nll_argument_errors(H):
    lib, p = H.lib(), abi.host_ptr()
    good = [p, p, p, p, p, p, 5, 2500]
    for i in range(5):                                        # images, run_recon, dyn, recon, rec_loss; d_recon is nullable
        args = list(good)
        args[i] = None
        assert lib.air_gauss_nll_fwd_bwd(*args, None) == H.EINVAL, i
    for i, bad in ((6, 0), (6, -1), (7, 0), (7, -3)):
        args = list(good)
        args[i] = bad
        assert lib.air_gauss_nll_fwd_bwd(*args, None) == H.EINVAL, (i, bad)
    assert "air_gauss_nll_fwd_bwd" in H.EXPORTED_SYMBOLS


def test_constructor_takes_the_likelihood_last():
    import inspect
    from air import air_model as am
    params = list(inspect.signature(am.AIRModel.__init__).parameters.values())
    assert params[-1].name == "likelihood" and params[-1].default == "bernoulli"
    assert am.AIRModel._LIKELIHOODS == {"bernoulli": 0, "gaussian": 1}
