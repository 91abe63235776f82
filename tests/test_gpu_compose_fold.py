"""air_write_fwd_bwd -- compose inside the graph-order write-backward launch -- against the two launches it stands for,
air_write_fwd and air_write_bwd with the batch means: every output bit for bit, the arrival count back at zero after every
call, and one host-side answer of the launcher and the name function for the descriptor pairs that keep two launches.
All calls go through the C ABI via ctypes."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi

KERNEL = "compose_write_bwd_graph_kernel"
Z = 50


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(H, B, N, Cc, w, seed, special=False):
    """records, windows, latents, images and targets of one step (numpy).  special: image 0 stops after step 1, image 1
    is never active, image 2 writes a tiny glimpse beyond a canvas corner (every canvas pixel clips to one window corner in
    both axes: all 4 C^2 terms in one corner slot), image 3 writes a glimpse that covers the canvas -- the workgroups of one
    launch then differ by orders of magnitude in work, and the owners arrive far apart."""
    rng = np.random.RandomState(seed)
    att = np.zeros((N, B, H.ATT_STRIDE), np.float32)
    att[:, :, H.ATT_S] = rng.uniform(0.08, 0.9, (N, B)); att[:, :, H.ATT_X] = rng.uniform(-0.9, 0.9, (N, B))
    att[:, :, H.ATT_Y] = rng.uniform(-0.9, 0.9, (N, B)); att[:, :, H.ATT_Z] = rng.uniform(0.2, 1.0, (N, B))
    for k in (H.ATT_KL_Z, H.ATT_KL_SCALE, H.ATT_KL_SHIFT):
        att[:, :, k] = rng.uniform(0.0, 3.0, (N, B))
    att[:, :, H.ATT_KL_VAE] = -5.0                                   # (an output: written for every step)
    alive = np.cumprod(rng.uniform(0, 1, (N, B)) < 0.75, axis=0).astype(np.float32)
    if special:
        assert B >= 5 and N >= 3
        alive[:, 0] = 0.0; alive[0, 0] = 1.0
        alive[:, 1] = 0.0
        alive[:, 2:5] = 1.0
        att[0, 2, H.ATT_S], att[0, 2, H.ATT_X], att[0, 2, H.ATT_Y] = 0.1, 1.3, 1.3
        att[0, 3, H.ATT_S], att[0, 3, H.ATT_X], att[0, 3, H.ATT_Y] = 1.0, 0.0, 0.0
    att[:, :, H.ATT_MASK] = alive
    att[1:, :, H.ATT_MASK_PREV] = alive[:-1]; att[0, :, H.ATT_MASK_PREV] = 1.0
    dyn = np.zeros(H.DYN_COUNT, np.float32)
    dyn[H.DYN_VAE_PV], dyn[H.DYN_GRAD_SCALE] = 1.0, 1.0 / B
    return dict(att=att, dyn=dyn,
                vrec=rng.uniform(0.05, 0.95, (N, B, w * w)).astype(np.float32),
                ml=rng.uniform(-1, 1, (N, B, 2 * Z)).astype(np.float32),
                images=(rng.uniform(0, 1, (B, Cc * Cc)) * (rng.uniform(0, 1, (B, Cc * Cc)) < 0.2)).astype(np.float32),
                targets=rng.randint(0, N + 1, B).astype(np.int32))


OUTPUTS = ("recon", "rec_loss", "run_loss", "run_digits", "loss_item", "att", "d_recon", "d_gen_pre", "d_gen_pre16",
           "d_sxy_write", "scalars")


def _run(H, inp, B, N, Cc, w, arrive=None):
    """one step on fresh output buffers (every word starts as a value no kernel writes): through air_write_fwd_bwd when an
    arrival word is given, through air_write_fwd + air_write_bwd otherwise"""
    lib = H.lib()
    t = lambda a_, dt=torch.float32: torch.tensor(a_, dtype=dt, device="cuda")  # noqa: E731
    vrec, ml, img, dyn, att, tg = t(inp["vrec"]), t(inp["ml"]), t(inp["images"]), t(inp["dyn"]), t(inp["att"]), t(inp["targets"], torch.int32)
    recon, d_recon = torch.full((B, Cc * Cc), 7.0, device="cuda"), torch.full((B, Cc * Cc), 7.0, device="cuda")
    rec_loss, run_loss, loss_item, scal = (torch.full((n_,), 7.0, device="cuda") for n_ in (B, B, B, 4))
    digits = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    dgen, dsx = torch.full((N, B, w * w), 7.0, device="cuda"), torch.full((N, B, 4), 7.0, device="cuda")
    dgen16 = torch.full((N, B, w * w), 7, dtype=torch.int16, device="cuda")
    wf = H.WriteFwd(_p(vrec), _p(ml), _p(img), _p(dyn), _p(att), _p(recon), _p(rec_loss), _p(d_recon), _p(run_loss), _p(digits),
                    _p(loss_item), B, N, Cc, w, Z, None)
    wb = H.WriteBwd(_p(d_recon), _p(vrec), _p(att), _p(dgen), _p(dsx), B, N, Cc, w, 2, _p(loss_item), _p(tg), _p(digits), _p(scal),
                    _p(dgen16), None)
    if arrive is None:
        H.check(lib.air_write_fwd(C.byref(wf), _stream()), "air_write_fwd")
        H.check(lib.air_write_bwd(C.byref(wb), _stream()), "air_write_bwd")
    else:
        buf = C.create_string_buffer(96)
        H.check(lib.air_write_fwd_bwd_kernel_name(C.byref(wf), C.byref(wb), buf, 96), "air_write_fwd_bwd_kernel_name")
        assert buf.value.decode() == KERNEL
        H.check(lib.air_write_fwd_bwd(C.byref(wf), C.byref(wb), _p(arrive), _stream()), "air_write_fwd_bwd")
    torch.cuda.synchronize()
    if arrive is not None:
        assert int(arrive.item()) == 0
    return dict(recon=recon, rec_loss=rec_loss, run_loss=run_loss, run_digits=digits, loss_item=loss_item, att=att,
                d_recon=d_recon, d_gen_pre=dgen, d_gen_pre16=dgen16, d_sxy_write=dsx, scalars=scal[:2].clone())


def _same(ref, got):
    for k in OUTPUTS:
        assert torch.equal(ref[k], got[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("B,N,Cc,w,special", [(5, 3, 50, 28, True), (37, 4, 33, 17, False), (2, 1, 50, 28, False),
                                              (64, 3, 50, 28, False)])
def test_one_launch_equals_compose_then_write_backward(B, N, Cc, w, special):
    """uneven load (5 images: one stopped after step 1, one never active, one with all 4 C^2 terms in one corner slot, one
    covering the canvas); C * C no multiple of the workgroup and an odd window; one step; the arrival count of the
    benchmark's batch"""
    H = abi.gpu_hip()
    inp = _inputs(H, B, N, Cc, w, seed=B + Cc, special=special)
    ref = _run(H, inp, B, N, Cc, w)
    arrive = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = _run(H, inp, B, N, Cc, w, arrive=arrive)
    _same(ref, got)
    # the reference itself wrote everything: no output still holds what the buffers started with
    att_in = inp["att"]
    assert not bool((ref["att"][:, :, H.ATT_KL_VAE] == -5.0).any())
    assert torch.equal(ref["att"][:, :, :H.ATT_KL_VAE].cpu(), torch.tensor(att_in[:, :, :H.ATT_KL_VAE]))
    for k in ("recon", "d_recon", "rec_loss", "run_loss", "loss_item", "d_gen_pre", "d_sxy_write", "scalars"):
        assert not bool((ref[k] == 7.0).any()), k
    assert not bool((ref["run_digits"] == -7).any()) and not bool((ref["d_gen_pre16"] == 7).any())
    assert float(ref["d_gen_pre"].abs().max()) > 0
    if special:
        # the inactive items have no gradient; the glimpse beyond the corner puts everything on ONE window pixel
        assert float(ref["d_gen_pre"][1:, 0].abs().max()) == 0 and float(ref["d_gen_pre"][:, 1].abs().max()) == 0
        assert not bool((ref["d_gen_pre"][0, 2, 1:] != 0).any())
        assert ref["run_digits"].tolist()[:4] == [1, 0, 3, 3]


@pytest.mark.gpu
def test_two_calls_in_a_row_share_one_arrival_word():
    """the second call -- other inputs, the same arrival word -- gives the second step's batch means; the word is zero
    after each call (_run reads it)"""
    H = abi.gpu_hip()
    B, N, Cc, w = 5, 3, 50, 28
    arrive = torch.zeros(1, dtype=torch.int32, device="cuda")
    first = _inputs(H, B, N, Cc, w, seed=1, special=True)
    second = _inputs(H, B, N, Cc, w, seed=2)
    got1 = _run(H, first, B, N, Cc, w, arrive=arrive)
    got2 = _run(H, second, B, N, Cc, w, arrive=arrive)
    ref1, ref2 = _run(H, first, B, N, Cc, w), _run(H, second, B, N, Cc, w)
    _same(ref1, got1)
    _same(ref2, got2)
    assert not torch.equal(ref1["scalars"], ref2["scalars"])


def test_pairs_that_keep_two_launches_get_one_answer_from_both_functions():
    """host only: the launcher and the name function read one plan and touch no GPU for a pair they refuse (the pointers
    are never dereferenced).  16 steps of compose scratch do not fit over the term buffer; more items than CUs come with
    an order buffer; the exact and the carried backward, a forward without d_recon and a pair that is not one step have
    no such form either."""
    H = abi.hip()
    lib = H.lib()
    P = abi.host_ptr()
    Q = C.c_void_p(P.value + 64)

    def pair(B, N, Cc, w, literal=2, order=None, d_recon=P, bwd_d_recon=P):
        wf = H.WriteFwd(P, P, P, P, P, P, P, d_recon, P, P, P, B, N, Cc, w, Z, order)
        wb = H.WriteBwd(bwd_d_recon, P, P, P, P, B, N, Cc, w, literal, P, P, P, P, P, order)
        return wf, wb

    def answers(wf, wb):
        buf = C.create_string_buffer(b"untouched", 96)
        name_rc = lib.air_write_fwd_bwd_kernel_name(C.byref(wf), C.byref(wb), buf, 96)
        run_rc = lib.air_write_fwd_bwd(C.byref(wf), C.byref(wb), P, None)
        assert name_rc == run_rc
        assert buf.value == b"untouched"
        return run_rc

    assert answers(*pair(2, 16, 50, 28)) == H.ELIMIT
    assert answers(*pair(100, 3, 50, 28, order=P)) == H.ELIMIT
    assert answers(*pair(100, 3, 50, 28)) == H.ELIMIT
    assert answers(*pair(64, 3, 128, 28)) == H.ELIMIT                # one tap's terms at a time: no term buffer to lie over
    assert answers(*pair(64, 3, 50, 28, literal=0)) == H.EINVAL
    assert answers(*pair(64, 3, 50, 28, literal=4)) == H.EINVAL
    assert answers(*pair(64, 3, 50, 28, d_recon=None, bwd_d_recon=None)) == H.EINVAL
    assert answers(*pair(64, 3, 50, 28, bwd_d_recon=Q)) == H.EINVAL
    # ... and the pair of the benchmark's step has the form
    wf, wb = pair(64, 3, 50, 28)
    buf = C.create_string_buffer(96)
    assert lib.air_write_fwd_bwd_kernel_name(C.byref(wf), C.byref(wb), buf, 96) == 0 and buf.value.decode() == KERNEL
    assert lib.air_write_fwd_bwd(C.byref(wf), C.byref(wb), None, None) == H.EINVAL      # no arrival word
