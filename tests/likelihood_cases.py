"""Inputs and fp64 references of the Gaussian-likelihood tests (tests/test_likelihood_cases.py on the CPU,
tests/test_gpu_likelihood.py on the GPU): the compose cases of tests/step_limit_cases.py under AIR_LIK_GAUSSIAN.

With R the fp64 running reconstruction, r = clip(R, 0, 1), x the image, sigma = dyn[AIR_DYN_LIK_STD], gsc =
dyn[AIR_DYN_GRAD_SCALE] and D = C * C (include/air_hip.h, above air_write_fwd_t):
    rec_loss[b] = (0.5 / sigma^2) * sum_p (x_p - r_p)^2 + D * (log sigma + 0.5 log 2 pi)
    d_recon[b, p] = (0 <= R <= 1) ? gsc * (r_p - x_p) / sigma^2 : 0"""
import functools

import numpy as np

import step_limit_cases as slc
from air import _hip as H

# canvases below and above the 4096-pixel prefetch threshold of the compose kernel, Z below and above one wave
COMPOSE_CASES = [(33, 7, 130), (50, 28, 50), (65, 32, 130)]
MASKED_IMAGE = 1          # the image of the variant case whose steps are all masked out: R == 0 on the whole image


def gaussian_nll(x, r, sigma):
    """[B] from [B, D] arrays, in the dtype of the inputs (float64 in every caller)"""
    D = x.shape[1]
    return (0.5 / sigma ** 2) * np.sum((x - r) ** 2, axis=1) + D * (np.log(sigma) + 0.5 * np.log(2.0 * np.pi))


def gaussian_reference(case, ref):
    """the Gaussian rec_loss / loss_item / d_recon of a compose case from its fp64 reference (slc.write_reference)"""
    f = np.float64
    x, r, R = case["images"].astype(f), ref["recon"], ref["R"]
    sigma, gsc = f(case["dyn"][H.DYN_LIK_STD]), f(case["dyn"][H.DYN_GRAD_SCALE])
    rec_loss = gaussian_nll(x, r, sigma)
    passes = (R >= 0.0) & (R <= 1.0)                         # Minimum / Maximum pass their gradient at ties
    d_recon = np.where(passes, gsc * (r - x) / sigma ** 2, 0.0)
    return dict(rec_loss=rec_loss, loss_item=ref["run_loss"] + rec_loss, d_recon=d_recon, passes=passes, sigma=sigma, gsc=gsc)


@functools.lru_cache(maxsize=None)
def compose_case_and_reference(C, w, Z):
    """(case, fp64 reference, Gaussian reference) of a compose case: shared, read-only"""
    case, ref = slc.write_case_and_reference(C, w, Z)
    return case, ref, gaussian_reference(case, ref)


@functools.lru_cache(maxsize=None)
def masked_case_and_reference():
    """(33, 7, 130) with ATT_MASK of image 1 zero at every step: no step writes, R = 0 on the whole image, and the tie at 0
    passes the clip's gradient.  The reference is slc.write_reference on the modified case."""
    base = slc.write_case(*COMPOSE_CASES[0])
    att = base["att"].copy()
    att[:, MASKED_IMAGE, H.ATT_MASK] = 0.0
    case = dict(base, att=att)
    ref = slc.write_reference(case)
    return case, ref, gaussian_reference(case, ref)
