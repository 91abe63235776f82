"""The kernels around the train step through the C ABI at their edges: the input queue and the row gather
(csrc/air_input.hip), air_summaries (csrc/air_summaries.hip), air_scene_records and air_render (csrc/air_generate.hip).
Case tables, inputs and references: tests/around_step_cases.py, pinned on the CPU by tests/test_around_step_cases.py.

The conventions are those of tests/test_gpu_pointwise_edges.py, whose helpers are used: a float input lies between NaN pads
and is NaN in every field its kernel has no business with, an integer input between out-of-range pads; an output starts as
sentinels between guard bands, which must be bit-identical afterwards, while every element of the written region must have
been written; no input changes; each launch (for the queue: each whole schedule of launches) runs twice on buffers of its
own and the two results are bit-identical.  Each test collects its failing cases and asserts at the end that there are none,
and prints the largest error / bound per quantity where a float tolerance applies (recorded in DESIGN.md section 39)."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import around_step_cases as asc
import pointwise_edge_cases as pec
import step_limit_cases as slc
from test_gpu_gemm_edges import DEV, SENT16, SENT32
from test_gpu_pointwise_edges import (_adr, _close, _Dense, _Flat, _Ints, _mat, _note, _report, _same_bits, _stream, _tagged, _twice,
                                      _values)

pytestmark = pytest.mark.gpu

SENT64 = -0x5A5A5A5A5A5A5A5B                      # the guards of the queue's int64 state
STATE_GUARD = 8


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


class _IntFlat(_Flat):
    """n int32 between GUARD sentinels; init: what the body holds before the launch (the queue image)"""

    def __init__(self, n, init=None):
        super().__init__(n)
        if init is not None:
            self.t[self.e:self.e + n] = torch.from_numpy(np.ascontiguousarray(init, np.int32)).to(DEV)

    def device_body(self):
        return self.t[self.e:self.e + self.n]

    def ints(self, bad, name):
        problems, body = self.check()
        bad += ["%s: %s" % (name, p) for p in problems]
        return body.view(np.int32)


def _untouched(outputs):
    """after a refused call: every output buffer still holds nothing but its sentinel"""
    torch.cuda.synchronize()
    return all((o.t == int(o.sent if hasattr(o, "sent") else SENT32)).all().item() for o in outputs)


# ---- 1. the shuffle queue -----------------------------------------------------------------------------------------------
def _run_queue(H, geometry, seed, schedule, start=None):
    """one schedule of dequeues on buffers of its own; start: (state, queue image) written into them, None: air_shuffle_batch_init"""
    cap, batch, mad, n_rec = geometry
    lib = H.lib()
    q = _IntFlat(cap, None if start is None else start[1])
    st = torch.full((2 * STATE_GUARD + 2,), SENT64, dtype=torch.int64, device=DEV)
    if start is not None:
        st[STATE_GUARD:STATE_GUARD + 2] = torch.tensor(start[0], dtype=torch.int64)
    pk = _IntFlat(batch)
    many = _IntFlat(max(n for kind, n in schedule if kind == "many") * batch)
    a = H.ShuffleBatch(q.ptr, st.data_ptr() + 8 * STATE_GUARD, pk.ptr, cap, batch, mad, n_rec, seed)
    if start is None:
        H.check(lib.air_shuffle_batch_init(C.byref(a), _stream()), "air_shuffle_batch_init")
    got, picks_kept = [], True
    for kind, n in schedule:
        if kind == "single":
            for _ in range(n):
                H.check(lib.air_shuffle_batch_dequeue(C.byref(a), _stream()), "air_shuffle_batch_dequeue")
                got.append(pk.device_body().clone().view(1, batch))
        else:
            before = pk.t.clone()
            H.check(lib.air_shuffle_batch_dequeue_many(C.byref(a), n, many.ptr, _stream()), "air_shuffle_batch_dequeue_many")
            picks_kept = picks_kept and torch.equal(pk.t, before)
            got.append(many.device_body().clone().view(n, batch))
    torch.cuda.synchronize()
    return dict(picks=torch.cat(got).cpu().numpy(), q=q, pk=pk, many=many, state=st.cpu().numpy(), picks_kept=picks_kept)


def _check_queue(H, geometry, seed, schedule, start=None):
    cap, batch = geometry[:2]
    want_picks, want_q, want_state = asc.queue_model(geometry, seed, schedule, None if start is None else (start[0], tuple(start[1])))
    a, b = _run_queue(H, geometry, seed, schedule, start), _run_queue(H, geometry, seed, schedule, start)
    bad = []
    if not (np.array_equal(a["picks"], b["picks"]) and np.array_equal(a["state"], b["state"]) and
            all(np.array_equal(a[k].host(), b[k].host()) for k in ("q", "pk", "many"))):
        bad.append("two runs differ in their bits")
    if a["picks"].shape != want_picks.shape or not np.array_equal(a["picks"], want_picks):
        rows = np.flatnonzero((a["picks"] != want_picks).any(axis=1)) if a["picks"].shape == want_picks.shape else []
        bad.append("picks differ from the literal queue%s" % (", first in dequeue %d" % rows[0] if len(rows) else ""))
    image = a["q"].ints(bad, "queue")
    if not np.array_equal(image, want_q):
        bad.append("queue image: %d slots differ from the literal queue's" % int((image != want_q).sum()))
    a["pk"].ints(bad, "picks")
    a["many"].ints(bad, "picks_out")
    if not a["picks_kept"]:
        bad.append("dequeue_many wrote q->picks")
    s = a["state"]
    if (s[:STATE_GUARD] != SENT64).any() or (s[STATE_GUARD + 2:] != SENT64).any():
        bad.append("the guards of state written")
    if tuple(int(v) for v in s[STATE_GUARD:STATE_GUARD + 2]) != want_state:
        bad.append("state %s, the literal queue's %s" % (s[STATE_GUARD:STATE_GUARD + 2].tolist(), list(want_state)))
    return bad


@pytest.mark.parametrize("geometry", asc.QUEUE_GEOMETRIES, ids=lambda g: "-".join(map(str, g)))
def test_queue_equals_the_literal_queue_in_both_resolvers(H, geometry):
    """12 single dequeues, one dequeue_many of 5, 3 single ones: picks, the queue image afterwards and state equal the
    literal pop-and-swap queue exactly -- the generic resolver (64 < batch <= 1024: never run on a device before) at 68, 128,
    256 and 1024 picks, capacity == batch, n_records of 1 and below batch, the two geometries on the 48 KB limit; guard
    bands behind queue, picks and picks_out, q->picks untouched by dequeue_many"""
    cap, batch = geometry[:2]
    bad = _check_queue(H, geometry, asc.QUEUE_SEED, asc.QUEUE_SCHEDULE)
    want_state = (cap + 20 * batch, 20)
    assert asc.queue_model(geometry, asc.QUEUE_SEED, asc.QUEUE_SCHEDULE)[2] == want_state
    assert not bad, "\n".join(bad)


def test_queue_with_stream_position_and_dequeue_number_past_32_bits(H):
    """state = [2^32 + 5, 2^32 - 2] and an arbitrary queue image written into the buffers: four single dequeues across the
    wrap of the counter's low word, then one dequeue_many of 3 -- the counter's high word and pos % n_records in 64 bits"""
    start = (asc.LARGE_STATE, asc.large_state_queue())
    bad = _check_queue(H, asc.LARGE_GEOMETRY, asc.LARGE_SEED, asc.LARGE_SCHEDULE, start)
    assert not bad, "\n".join(bad)


# ---- 2. air_batch_gather --------------------------------------------------------------------------------------------------
def _gather_buffers(c, x):
    img = _Dense(x["images"])
    dig = _Ints(x["digits"]) if c["mode"] != "none" else None
    pk = _Ints(x["picks"], pad=c["records"])                  # one past the last record
    o = dict(out_images=_mat(c["batch"], c["D"]), out_digits=_IntFlat(c["batch"]) if c["mode"] == "both" else None)
    return img, dig, pk, o


def test_batch_gather_at_slice_edges_with_and_without_digits(H):
    """D = 4 (one float4) .. 16388, D / 4 = 1024 (one slice of a row) against 1025 (two), batch 1, 3 and 64, tables of 1, 5
    and 300 records, picks with the first and the last record and repeats; digits and out_digits, digits alone, neither:
    exactly images[picks] and digits[picks]"""
    failures = []
    for c in asc.GATHER_CASES:
        x = asc.gather_inputs(c)

        def launch():
            img, dig, pk, o = _gather_buffers(c, x)
            assert img.adr % 16 == 0 and o["out_images"].ptr % 16 == 0
            H.check(H.lib().air_batch_gather(img.adr, _adr(dig), pk.adr, o["out_images"].ptr, _adr(o["out_digits"]), c["batch"], c["D"],
                                             _stream()), "air_batch_gather")
            return o, (img, dig, pk)
        out, bad = _twice(launch)
        _same_bits(bad, "out_images against images[picks]", _values(bad, "out_images", out["out_images"]), x["images"][x["picks"]])
        if c["mode"] == "both":
            _same_bits(bad, "out_digits against digits[picks]", out["out_digits"].ints(bad, "out_digits"), x["digits"][x["picks"]])
        failures += _tagged(c, bad)
    _report(failures, "batch_gather")


def test_batch_gather_refuses_what_it_cannot_copy(H):
    c = dict(D=8, batch=3, records=5, mode="both")
    x = asc.gather_inputs(c)
    img, dig, pk, o = _gather_buffers(c, x)
    call = lambda images, digits, D: H.lib().air_batch_gather(images, digits, pk.adr, o["out_images"].ptr, o["out_digits"].ptr,  # noqa: E731
                                                              c["batch"], D, _stream())
    assert call(img.adr, dig.adr, 6) == H.EALIGN                               # rows are copied in 16-byte pieces
    assert call(img.adr + 4, dig.adr, 8) == H.EALIGN
    assert call(img.adr, None, 8) == H.EINVAL                                  # out_digits without digits
    assert _untouched(o.values()) and not img.changed() and not dig.changed() and not pk.changed()


# ---- 3. air_summaries -----------------------------------------------------------------------------------------------------
def _summary_struct(H, ins, out, B, N, md):
    return H.Summaries(ins["att"].adr, ins["targets"].adr, ins["digits"].adr, ins["rec_loss"].adr, ins["loss_item"].adr,
                       ins["scalars"].adr, out.ptr, B, N, md)


def _summary_buffers(x):
    return dict(att=_Dense(x["att"]), targets=_Ints(x["targets"]), digits=_Ints(x["digits"]), rec_loss=_Dense(x["rec_loss"]),
                loss_item=_Dense(x["loss_item"]), scalars=_Dense(x["scalars"]))


def test_summaries_against_the_restatement_without_a_model(H):
    """N = 1, 3, 16; max_digits = 0, 2, 6 (the _all_dig slot directly behind the last digit group); B = 1 .. 1000 on both sides
    of one wave and of one workgroup; a loop that stopped at T' < N with NaN in every value slot of the rows behind T' (the
    result is the reference's zero padding); targets above max_digits; empty groups (NaN where the reference has NaN):
    oracle.summaries.summaries on the [B, T'] stacks, rtol 2e-7, atol 0"""
    failures = []
    for c in asc.SUMMARY_CASES:
        B, N, md = c["B"], c["N"], c["max_digits"]
        x = asc.summary_inputs(c)
        ref = asc.summary_reference(c, x)
        n = H.lib().air_summaries_count(N, md)
        assert ref.shape == (n,)

        def launch():
            ins = _summary_buffers(x)
            o = dict(out=_Flat(n))
            H.check(H.lib().air_summaries(C.byref(_summary_struct(H, ins, o["out"], B, N, md)), _stream()), "air_summaries")
            return o, ins.values()
        out, bad = _twice(launch)
        problems, got = out["out"].check()
        bad += problems
        _same_bits(bad, "loss and accuracy against scalars", got[:2], x["scalars"])
        rows = 2 + 4 * (md + 2)
        for key, sl in (("summaries/post-loop rows", slice(2, rows)), ("summaries/per-step rows", slice(rows, n))):
            r = asc.summary_ratio(got[sl], ref[sl])
            _note(key, r)
            if not r <= 1.0:
                k = np.flatnonzero(~((got[sl] == ref[sl]) | (np.isnan(got[sl]) & np.isnan(ref[sl]))))
                bad.append("%s: error / bound = %.3g; first at entry %d: %r, reference %r" % (key, r, sl.start + k[0], got[sl][k[0]], ref[sl][k[0]]))
        failures += _tagged(c, bad)
    _report(failures, "summaries")


def test_summaries_refuses_what_is_past_its_limits(H):
    c = dict(B=4, N=3, max_digits=2, T=3)
    ins = _summary_buffers(asc.summary_inputs(c))
    out = _Flat(H.lib().air_summaries_count(16, 6))
    call = lambda B, N, md: H.lib().air_summaries(C.byref(_summary_struct(H, ins, out, B, N, md)), _stream())  # noqa: E731
    assert call(4, 17, 2) == H.ELIMIT and call(4, 3, 7) == H.ELIMIT and call(0, 3, 2) == H.EINVAL
    assert _untouched([out]) and not any(v.changed() for v in ins.values())


# ---- 4. air_scene_records -------------------------------------------------------------------------------------------------
SCENE_SOURCES = ("scale_src", "shift_src", "z_src", "pres_src")


def _scene_buffers(c, x):
    rows = c["N"] * c["B"]
    ins = {k: _Dense(x[k]) for k in SCENE_SOURCES + ("dyn",)}
    return ins, dict(att=_mat(rows, 16), z=_mat(rows, c["ldz"]), z16=_mat(rows, c["ldz"], bits=16))


def _scene_struct(H, c, ins, o, att=None, **kw):
    f = dict(B=c["B"], N=c["N"], Z=c["Z"], ldz=c["ldz"], given=c["given"])
    f.update(kw)
    return H.SceneRecords(ins["scale_src"].adr, ins["shift_src"].adr, ins["z_src"].adr, ins["pres_src"].adr, ins["dyn"].adr,
                          o["att"].ptr if att is None else att, o["z"].ptr, o["z16"].ptr if c["z16"] else None,
                          f["B"], f["N"], f["Z"], f["ldz"], f["given"])


def test_scene_records_against_float64_sampled_and_given(H):
    """the smallest launch; 16 steps with padded latent rows and the twin; N < 16 with tight rows; a grid sized by B (two
    workgroups); B past one workgroup with everything on -- each with given = 0 and 1, stop plans of steps 0, (N - 1) / 2 and
    N - 1 repeated over B: the header's formulas in float64 on the fp32 inputs"""
    failures = []
    for c in asc.SCENE_CASES:
        B, N, Z, ldz, given = c["B"], c["N"], c["Z"], c["ldz"], c["given"]
        x = asc.scene_inputs(c)
        ref = asc.scene_reference(c, x)

        def launch():
            ins, o = _scene_buffers(c, x)
            assert o["att"].ptr % 16 == 0
            H.check(H.lib().air_scene_records(C.byref(_scene_struct(H, c, ins, o)), _stream()), "air_scene_records")
            return o, ins.values()
        out, bad = _twice(launch)
        att = _values(bad, "att", out["att"]).reshape(N, B, H.ATT_STRIDE)
        z2 = _values(bad, "z", out["z"])
        z = z2.reshape(N, B, ldz)
        if not (np.isfinite(att).all() and np.isfinite(z).all()):
            bad.append("a value that is not finite")
        for name, k in asc.att_close_columns():
            r = asc.att_ratio(att[..., k], ref["att"][..., k])
            _note("scene_records/" + name, r)
            if not r <= 1.0:
                bad.append("%s: error / bound = %.3g" % (name, r))
        for name in ("Z", "MASK_PREV", "MASK"):
            k = getattr(H, "ATT_" + name)
            _same_bits(bad, name + " against the reference", att[..., k], ref["att"][..., k].astype(np.float32))
        _same_bits(bad, "MASK_PREV[t] against MASK[t - 1]", att[1:, :, H.ATT_MASK_PREV], att[:-1, :, H.ATT_MASK])
        _same_bits(bad, "MASK_PREV[0] against 1", att[0, :, H.ATT_MASK_PREV], np.ones(B, np.float32))
        if att[..., list(asc.ATT_ZERO)].any():
            bad.append("ZPROB, a KL slot or ST_BACK + 3 is not 0")
        if given:
            for name, src in (("S", x["scale_src"]), ("X", x["shift_src"][..., 0]), ("Y", x["shift_src"][..., 1]), ("Z", x["pres_src"])):
                _same_bits(bad, name + " against its source", att[..., getattr(H, "ATT_" + name)], src)
            if att[..., H.ATT_ZPRE].any():
                bad.append("ZPRE is not 0")
            _same_bits(bad, "latents against their source", z[..., :Z], x["z_src"])
        else:
            _close(bad, "scene_records/z", z[..., :Z], ref["z"][..., :Z], pec.REPARAM_FWD_TOL)
        if z[..., Z:].view(np.int32).any():
            bad.append("a pad column of z is not +0")
        if c["z16"]:
            _same_bits(bad, "z16 against bf16 of the written z", _values(bad, "z16", out["z16"]), slc.bf16_rne(z2).view(np.int16))
        elif (out["z16"].host() != SENT16).any():
            bad.append("no twin asked for, and the twin buffer was written")
        failures += _tagged(c, bad)
    _report(failures, "scene_records")


def test_scene_records_refuses_misaligned_records_and_bad_extents(H):
    c = dict(B=3, N=5, Z=50, ldz=50, z16=True, given=1)
    ins, o = _scene_buffers(c, asc.scene_inputs(c))
    call = lambda **kw: H.lib().air_scene_records(C.byref(_scene_struct(H, c, ins, o, **kw)), _stream())  # noqa: E731
    assert call(att=o["att"].ptr + 4) == H.EALIGN
    assert call(N=17) == H.ELIMIT
    assert call(ldz=49) == H.EINVAL
    assert _untouched(o.values()) and not any(v.changed() for v in ins.values())


# ---- 5. air_render --------------------------------------------------------------------------------------------------------
def _write_fwd_recon(H, case):
    """air_write_fwd's recon and run_digits on the same records and windows (plain buffers: that kernel's guards are
    tests/test_gpu_step_limits.py's business); Z = 1 and blank images: neither enters the reconstruction"""
    B, N, Cc, w = case["B"], case["N"], case["C"], case["w"]
    t = lambda a: torch.tensor(np.ascontiguousarray(a), device=DEV)  # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())  # noqa: E731
    vrec, att, dyn = t(case["vrec"]), t(case["att"]), t(slc.dyn_vector(B))
    ml, images = torch.zeros(N, B, 2, device=DEV), torch.zeros(B, Cc * Cc, device=DEV)
    recon = torch.full((B, Cc * Cc), float("nan"), device=DEV)
    rec_loss, run_loss, loss_item = (torch.full((B,), float("nan"), device=DEV) for _ in range(3))
    digits = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    wf = H.WriteFwd(p(vrec), p(ml), p(images), p(dyn), p(att), p(recon), p(rec_loss), None, p(run_loss), p(digits), p(loss_item),
                    B, N, Cc, w, 1, None)
    rc = H.lib().air_write_fwd(C.byref(wf), _stream())
    torch.cuda.synchronize()
    return rc, recon.cpu().numpy(), digits.cpu().numpy()


def _render_struct(H, ins, o, B, N, Cc, w):
    return H.Render(ins["vrec"].adr, ins["att"].adr, o["canvas"].ptr, o["num_digits"].ptr, B, N, Cc, w)


def test_render_sixteen_steps_at_small_and_odd_canvases(H):
    """the 16-step compose cases (C = 50, 51, 64, 65, 33) and C = 7, 2 and 31 with windows of 2 and 5 pixels -- C C < 1024,
    1024 % C != 0, the smallest shape admitted: the pixel walk of render_kernel.  The canvas within 2e-5 of the clipped
    float64 running reconstruction, num_digits exact, and the bits of air_write_fwd's recon on the same records; the records
    NaN in every slot but S, X, Y, Z and MASK"""
    failures = []
    for Cc, w in asc.RENDER_CASES:
        case, ref = asc.render_case_and_reference(Cc, w)
        B, N = case["B"], case["N"]
        att = asc.render_att(case["att"])

        def launch():
            ins = dict(vrec=_Dense(case["vrec"]), att=_Dense(att))
            o = dict(canvas=_mat(B, Cc * Cc), num_digits=_IntFlat(B))
            H.check(H.lib().air_render(C.byref(_render_struct(H, ins, o, B, N, Cc, w)), _stream()), "air_render")
            return o, ins.values()
        out, bad = _twice(launch)
        canvas = _values(bad, "canvas", out["canvas"])
        _close(bad, "render/canvas", canvas, ref["canvas"], (0.0, asc.RENDER_TOL))
        _same_bits(bad, "num_digits", out["num_digits"].ints(bad, "num_digits"), ref["digits"])
        rc, recon, run_digits = _write_fwd_recon(H, case)
        if rc == 0:
            _same_bits(bad, "canvas against air_write_fwd's recon", canvas, recon)
            _same_bits(bad, "num_digits against air_write_fwd's run_digits", out["num_digits"].ints([], ""), run_digits)
        elif rc not in (H.ELIMIT,):
            bad.append("air_write_fwd returned %d" % rc)
        failures += _tagged("C=%d w=%d" % (Cc, w), bad)
    _report(failures, "render")


def test_render_refuses_degenerate_shapes(H):
    case, _ = asc.render_case_and_reference(7, 2)
    B, N = case["B"], case["N"]
    ins = dict(vrec=_Dense(case["vrec"]), att=_Dense(asc.render_att(case["att"])))
    o = dict(canvas=_mat(B, 49), num_digits=_IntFlat(B))
    call = lambda N_, C_, w_: H.lib().air_render(C.byref(_render_struct(H, ins, o, B, N_, C_, w_)), _stream())  # noqa: E731
    assert call(N, 1, 2) == H.EINVAL and call(N, 7, 1) == H.EINVAL
    assert call(17, 7, 2) == H.ELIMIT
    assert _untouched(o.values()) and not any(v.changed() for v in ins.values())
