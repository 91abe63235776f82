"""air_write_bwd in its launch forms -- the exact adjoint (literal 0), the graph order (2) and the carried order (4), each at
canvases that keep all four taps' terms resident and at one that stages a tap at a time -- pinned for what the forms have
in common: the optional outputs (batch means, bf16 twin, launch order) move no bit of the gradients, the batch means are
the same bits in every form and are written by a workgroup whose own item is inactive, nothing lands outside the outputs,
and nothing else is written.  All calls go through the C ABI via ctypes; every launch of a (shape, literal) pair runs once
and is shared by the tests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abi_check as abi

# (B, N, C, w): all taps resident at C = 33, 40 and 50, one tap per pass at 71
SHAPES = [(3, 2, 33, 17), (4, 3, 50, 28), (3, 2, 71, 28), (3, 2, 40, 9)]
LITERALS = [0, 2, 4]
SENT, SENT16 = 7.0, 0x1234


def _p(t, offset=0):
    return C.c_void_p(t.data_ptr() + offset * t.element_size()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf16_rne(a):
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def _inputs(B, N, Cc, w):
    """the recipe of test_write_bwd_graph_order_matches_oracle_all_canvas_sizes: poles of 1e7 in d loss / d canvas, one
    glimpse in a canvas corner, one covering the canvas; item (t = 0, b = 0) and the last step of the last image inactive"""
    H = abi.gpu_hip()
    rng = np.random.RandomState(Cc * 3 + w + N)
    s = rng.uniform(0.12, 0.6, (N, B)).astype(np.float32)
    x = rng.uniform(-0.8, 0.8, (N, B)).astype(np.float32)
    y = rng.uniform(-0.8, 0.8, (N, B)).astype(np.float32)
    s[0, 1], x[0, 1], y[0, 1] = 0.3, -0.95, 0.9
    s[0, 2], x[0, 2], y[0, 2] = 0.97, 0.02, -0.01
    z = rng.uniform(0.05, 1.0, (N, B)).astype(np.float32)
    mask = np.ones((N, B), np.float32)
    mask[0, 0] = 0.0
    mask[N - 1, B - 1] = 0.0
    att = np.zeros((N, B, H.ATT_STRIDE), np.float32)
    att[:, :, H.ATT_S], att[:, :, H.ATT_X], att[:, :, H.ATT_Y], att[:, :, H.ATT_Z] = s, x, y, z
    att[:, :, H.ATT_MASK] = mask
    g = (rng.randn(B, Cc * Cc) * np.where(rng.uniform(size=(B, Cc * Cc)) < 0.08, 1e7, 1e-2)).astype(np.float32)
    vrec = rng.uniform(0.01, 0.99, (N, B, w * w)).astype(np.float32)
    loss_item = rng.uniform(50.0, 900.0, B).astype(np.float32)
    targets = rng.randint(0, N + 1, B).astype(np.int32)
    digits = targets.copy()
    digits[B - 1] += 1                                       # k = B - 1 images counted right
    dev = {k: torch.tensor(v, device="cuda") for k, v in dict(att=att, g=g, vrec=vrec, loss_item=loss_item, targets=targets,
                                                              digits=digits).items()}
    return dict(mask=mask, loss_item=loss_item, k=B - 1, dev=dev)


def _launch(H, shape, literal, fin, twin, order, guard):
    """one air_write_bwd on fresh buffers that start as sentinels; guard: one extra item of sentinels before and after every
    output.  Returns the whole buffers (numpy) and the scalars."""
    B, N, Cc, w = shape
    d = _inputs(*shape)["dev"]
    ww, items, pad = w * w, N * B, 1 if guard else 0
    dgen = torch.full(((items + 2 * pad) * ww,), SENT, device="cuda")
    dsx = torch.full(((items + 2 * pad) * 4,), SENT, device="cuda")
    dgen16 = torch.full(((items + 2 * pad) * ww,), SENT16, dtype=torch.int16, device="cuda") if twin else None
    scal = torch.full((4,), SENT, device="cuda") if fin else None
    perm = torch.arange(items - 1, -1, -1, dtype=torch.int32, device="cuda") if order else None
    wb = H.WriteBwd(_p(d["g"]), _p(d["vrec"]), _p(d["att"]), _p(dgen, pad * ww), _p(dsx, pad * 4), B, N, Cc, w, literal,
                    _p(d["loss_item"]) if fin else None, _p(d["targets"]) if fin else None, _p(d["digits"]) if fin else None,
                    _p(scal), _p(dgen16, pad * ww) if twin else None, _p(perm))
    name = C.create_string_buffer(96)
    H.check(H.lib().air_write_bwd_kernel_name(C.byref(wb), name, 96))
    want = "write_bwd_kernel" if literal == 0 else \
        "write_bwd_%s_kernel<%s>" % ({2: "graph", 4: "carried"}[literal], "true" if Cc in (33, 40, 50) else "false")
    assert name.value.decode() == want
    H.check(H.lib().air_write_bwd(C.byref(wb), _stream()), "air_write_bwd")
    torch.cuda.synchronize()
    return dict(dgen=dgen.cpu().numpy(), dsx=dsx.cpu().numpy(),
                dgen16=dgen16.cpu().numpy().view(np.uint16) if twin else None,
                scal=scal.cpu().numpy() if fin else None)


@functools.lru_cache(maxsize=None)
def _forms(shape, literal):
    """the launches of one (shape, literal): `plain` (no batch means, no twin, no order, no guard), `full` (all of them, the
    reversed range as order where the literal has one, in guarded allocations) and, for the literals with an order, `means`
    (batch means and twin, no order)"""
    H = abi.gpu_hip()
    ordered = literal != 0
    out = dict(plain=_launch(H, shape, literal, fin=False, twin=False, order=False, guard=False),
               full=_launch(H, shape, literal, fin=True, twin=True, order=ordered, guard=True))
    if ordered:
        out["means"] = _launch(H, shape, literal, fin=True, twin=True, order=False, guard=False)
    return out


def _inside(buf, per, items):
    return buf[per:per * (items + 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("literal", LITERALS)
@pytest.mark.parametrize("shape", SHAPES)
def test_optional_outputs_move_no_bit(shape, literal):
    """batch means + bf16 twin + the reversed launch order (literals 2 and 4: the launcher accepts `order` for both and both
    bodies honour it) against the plain call: d_gen_pre and d_sxy_write byte for byte, the twin the RNE bf16 of d_gen_pre"""
    B, N, Cc, w = shape
    f = _forms(shape, literal)
    plain = f["plain"]
    assert np.isfinite(plain["dgen"]).all() and np.isfinite(plain["dsx"]).all() and plain["dgen"].any()
    for k in ("full", "means") if literal else ("full",):
        got = f[k]
        pad = 1 if k == "full" else 0
        dgen = _inside(got["dgen"], w * w, N * B) if pad else got["dgen"]
        dsx = _inside(got["dsx"], 4, N * B) if pad else got["dsx"]
        d16 = _inside(got["dgen16"], w * w, N * B) if pad else got["dgen16"]
        assert dgen.tobytes() == plain["dgen"].tobytes(), k
        assert dsx.tobytes() == plain["dsx"].tobytes(), k
        assert np.array_equal(d16, _bf16_rne(plain["dgen"])), k


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_batch_means_are_the_same_bits_in_every_form(shape):
    """fin_scalars[0:2]: one loop and one air_block_sum4<16> in all three kernels -- byte-identical across the literals and
    with or without `order`; accuracy exactly k / B; written although the finishing workgroup's own item is inactive (item
    (0, 0) is the first workgroup's without `order` and the last workgroup's with the reversed one); fin_scalars[2:4] keep
    their sentinel"""
    B = shape[0]
    inp = _inputs(*shape)
    assert inp["mask"][0, 0] == 0.0 and inp["mask"][-1, -1] == 0.0
    scal = [_forms(shape, lit)[k]["scal"] for lit in LITERALS for k in ("full", "means") if k in _forms(shape, lit)]
    assert len(scal) == 5
    for s4 in scal:
        assert s4[:2].tobytes() == scal[0][:2].tobytes()
        assert s4[2:].tobytes() == np.full(2, SENT, np.float32).tobytes()
    assert scal[0][1] == np.float32(inp["k"]) / np.float32(B)
    mean = float(inp["loss_item"].astype(np.float64).mean())
    assert abs(float(scal[0][0]) - mean) <= 1e-6 * mean


@pytest.mark.gpu
@pytest.mark.parametrize("literal", LITERALS)
@pytest.mark.parametrize("shape", SHAPES)
def test_outputs_stay_inside_their_allocations(shape, literal):
    """one extra item of 7.0 / 0x1234 before and after d_gen_pre, d_gen_pre16 and d_sxy_write: every sentinel survives, the
    inactive items are exact zeros in all three outputs (the inside equals the unguarded launch: the test above)"""
    B, N, Cc, w = shape
    full = _forms(shape, literal)["full"]
    mask = _inputs(*shape)["mask"].reshape(-1)
    for key, per, sent in (("dgen", w * w, np.float32(SENT)), ("dgen16", w * w, np.uint16(SENT16)), ("dsx", 4, np.float32(SENT))):
        buf = full[key]
        assert buf.size == per * (N * B + 2)
        assert (buf[:per] == sent).all() and (buf[-per:] == sent).all(), key
        inside = _inside(buf, per, N * B).reshape(N * B, per)
        for item in np.flatnonzero(mask == 0.0):
            assert inside[item].tobytes() == bytes(inside[item].nbytes), (key, item)
        assert inside[mask != 0.0].any(), key
