"""GPU tests of the localisation metrics (air_localization of include/air_hip.h, air/metrics.py).

The reference is the float64 restatement of tests/localization_cases.py.  Everything is compared BIT FOR BIT: every number
is a chain of correctly rounded float64 operations in the header's order, every decision a comparison of such numbers, and
the sums have one order.  Every buffer the kernel writes is guarded: sentinels in front of and behind every output, and
behind row k of the per-digit outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import localization_cases as lc

pytestmark = pytest.mark.gpu

GUARD = 8                                    # sentinel elements in front of and behind every output
FILL_I32, FILL_I64, FILL_F64 = -5, -(2 ** 40) - 5, -7.25
CASES = lc.gpu_cases()


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Guarded:
    """a device buffer of n elements between two rows of sentinels; `init` fills the payload"""

    def __init__(self, n, dtype, fill, init=None):
        self.n, self.fill = n, fill
        self.buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
        if init is not None:
            self.buf[GUARD:GUARD + n] = init
        self.view = self.buf[GUARD:GUARD + n]

    def payload(self):
        """the payload as numpy, after checking the sentinels"""
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == self.fill).all() and (host[GUARD + self.n:] == self.fill).all(), "a sentinel was overwritten"
        return host[GUARD:GUARD + self.n]


def run_case(H, case, per_digit=True, upto=None, rows_behind=2):
    """the chunks of `case` through air_localization, one call each on shared accumulators, stream-ordered
    -> ([(match, iou)] per chunk, counts, sums) as numpy; per_digit=False passes match = iou = NULL"""
    T, B, G = case["T"], case["B"], case["G"]
    counts = Guarded(lc.COUNTS + (G + 1) * (T + 1), torch.int64, FILL_I64, init=0)
    sums = Guarded(lc.SUMS, torch.float64, FILL_F64, init=0.0)
    keep, outs = [], []
    for ch in case["chunks"][:upto]:
        k = ch["k"]
        nbytes = H.lib().air_localization_workspace_bytes(T, B, k, G)
        assert nbytes == -(-k // lc.GROUP) * lc.SUMS * 8
        ws = Guarded(nbytes // 8, torch.float64, FILL_F64)
        # rows_behind: the per-digit outputs have rows beyond k, which must stay sentinels
        match = Guarded((k + rows_behind) * G, torch.int32, FILL_I32)
        iou = Guarded((k + rows_behind) * G, torch.float64, FILL_F64)
        d = {name: _dev(ch[name]) for name in ("att", "run_digits", "gt_count", "gt_positions", "gt_boxes")}
        a = H.Localization(*(H.ptr(d[name]) for name in ("att", "run_digits", "gt_count", "gt_positions", "gt_boxes")),
                           H.ptr(match.view) if per_digit else None, H.ptr(iou.view) if per_digit else None,
                           H.ptr(counts.view), H.ptr(sums.view), T, B, k, G, case["canvas_size"], case["tau"])
        H.launch("air_localization", torch.device("cuda"), C.byref(a), H.ptr(ws.view))
        keep.append((d, ws))
        outs.append((match, iou, k))
    torch.cuda.synchronize()
    for _, ws in keep:
        ws.payload()
    got = []
    for match, iou, k in outs:
        m, v = match.payload(), iou.payload()
        if per_digit:
            assert (m[k * G:] == FILL_I32).all() and (v[k * G:] == FILL_F64).all(), "a row >= k was written"
        else:
            assert (m == FILL_I32).all() and (v == FILL_F64).all()
        got.append((m[:k * G].reshape(k, G), v[:k * G].reshape(k, G)))
    return got, counts.payload(), sums.payload()


def check_case(H, name):
    case = CASES[name]
    want_out, want_c, want_s = lc.expected(name)
    got_out, got_c, got_s = run_case(H, case)
    print("%s: counts %s sums %s" % (name, got_c[:lc.COUNTS].tolist(), got_s.tolist()))
    for (gm, gv), (wm, wv) in zip(got_out, want_out):
        assert gm.dtype == wm.dtype and gm.tobytes() == wm.tobytes(), (name, gm, wm)
        assert gv.dtype == wv.dtype and gv.tobytes() == wv.tobytes(), (name, gv, wv)
    assert got_c.dtype == want_c.dtype and got_c.tobytes() == want_c.tobytes(), (name, got_c, want_c)
    assert got_s.dtype == want_s.dtype and got_s.tobytes() == want_s.tobytes(), (name, got_s.tolist(), want_s.tolist())
    return got_out, got_c, got_s


@pytest.mark.parametrize("name", ["t%d_g%d_k%d_b%d" % s for s in lc.SHAPES])
def test_kernel_equals_the_restatement(H, name):
    """(T, G, k, B) = (1, 1, 1, 1), (3, 2, 5, 8), (16, 16, 7, 7), (3, 2, 64, 64), (3, 2, 65, 70), (3, 2, 257, 260): one
    image; k < B; the limits; one full wave; a second wave; one image beyond the workgroup (a second group in the fold)"""
    check_case(H, name)


def test_every_branch_of_the_table(H):
    """(4, 3, 32, 32): ties, unmatched digits and objects, empty images, clamped counts, NaN records, a pair at tau, the
    greedy choice -- tests/test_localization_cases.py asserts the table holds each of them"""
    got_out, got_c, _ = check_case(H, "branches")
    at, match, iou = CASES["branches"]["planted"], got_out[0][0], got_out[0][1]
    assert match[at["tie_objects"]][0] == 0 and match[at["tie_digits"]].tolist()[:2] == [0, -1]
    assert match[at["nan"]].tolist()[:2] == [-1, 2] and match[at["greedy"]].tolist()[:2] == [-1, 0]
    assert iou[at["at_tau"]][0] == 0.5 and match[at["outside"]][0] == -1


def test_two_calls_accumulate(H):
    """k1 + k2 rows in two calls on the same accumulators = the restatement applied in the same two steps; the first call
    alone = its first step (so the second call added to what it found)"""
    check_case(H, "two_chunks")
    _, want_c, want_s = lc.expected("two_chunks", upto=1)
    _, got_c, got_s = run_case(H, CASES["two_chunks"], upto=1)
    assert got_c.tobytes() == want_c.tobytes() and got_s.tobytes() == want_s.tobytes()
    _, all_c, all_s = lc.expected("two_chunks")
    assert all_c[lc.IMAGES] == 8 and all_c.tobytes() != want_c.tobytes() and all_s.tobytes() != want_s.tobytes()


@pytest.mark.parametrize("name", ["branches", "t3_g2_k257_b260", "two_chunks"])
def test_without_per_digit_outputs_the_accumulators_are_the_same(H, name):
    _, want_c, want_s = lc.expected(name)
    _, got_c, got_s = run_case(H, CASES[name], per_digit=False)
    assert got_c.tobytes() == want_c.tobytes() and got_s.tobytes() == want_s.tobytes()


def test_the_same_inputs_give_the_same_bits(H):
    a, b = run_case(H, CASES["t3_g2_k257_b260"]), run_case(H, CASES["t3_g2_k257_b260"])
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


# -------------------------------------------------------------------------------------------------------------- the module
class _Pass:
    """what Localization reads of a model, with the records of a case's chunk where a forward would have left them"""

    def __init__(self, case, chunk):
        self.max_steps, self.batch_size, self.canvas_size = case["T"], case["B"], case["canvas_size"]
        self.input_images = torch.zeros(case["B"], case["canvas_size"] ** 2, device="cuda")
        self.att, self.run_digits = _dev(chunk["att"]), _dev(chunk["run_digits"])
        self.ensured = 0

    def _ensure(self):
        self.ensured += 1


def test_module_accumulates_resets_and_takes_both_layouts(H):
    from air.metrics import Localization
    case = CASES["two_chunks"]
    c0, c1 = case["chunks"]
    G = case["G"]
    model = _Pass(case, c0)
    loc = Localization(model, G, iou_threshold=case["tau"], per_digit=True)
    assert loc.names() == list(lc.NAMES)
    # chunk 0 as device tensors [k, G, 2], chunk 1 as numpy arrays [k, 2 G]
    loc.update(_dev(c0["gt_count"]), _dev(c0["gt_positions"]), _dev(c0["gt_boxes"]))
    model.att, model.run_digits = _dev(c1["att"]), _dev(c1["run_digits"])
    loc.update(c1["gt_count"], c1["gt_positions"].reshape(c1["k"], 2 * G), c1["gt_boxes"].reshape(c1["k"], 2 * G))
    assert model.ensured == 2
    out, want_c, want_s = lc.expected("two_chunks")
    assert loc.counts.cpu().numpy().tobytes() == want_c.tobytes() and loc.sums.cpu().numpy().tobytes() == want_s.tobytes()
    k1 = c1["k"]
    assert loc.match[:k1].cpu().numpy().tobytes() == out[1][0].tobytes() and loc.iou[:k1].cpu().numpy().tobytes() == out[1][1].tobytes()
    values = loc.values()
    assert values.is_cuda and values.dtype == torch.float64
    assert values.cpu().numpy().tobytes() == lc.derived(want_c, want_s).tobytes()
    into = torch.zeros(len(lc.NAMES), dtype=torch.float64, device="cuda")
    assert loc.values(into) is into and torch.equal(into, values)
    res = loc.result()
    assert [res[n] for n in lc.NAMES] == lc.derived(want_c, want_s).tolist()
    assert res["confusion"].tobytes() == lc.confusion(case, want_c).tobytes() and res["images"] == 8
    # reset() between calls: the second chunk alone, in the [k, 2 G] device layout, with k given for tensors of more rows
    loc.reset()
    assert np.isnan(loc.values().cpu().numpy()).all()                       # every denominator is zero
    pad = lambda a: _dev(np.concatenate([a.reshape(k1, -1), np.full((3, a.reshape(k1, -1).shape[1]), 9, np.int32)]))   # noqa: E731
    loc.update(pad(c1["gt_count"]).view(-1), pad(c1["gt_positions"]), pad(c1["gt_boxes"]), k=k1)
    counts, sums = lc.empty_accumulators(case)
    lc.apply_chunk(case, c1, counts, sums)
    assert loc.counts.cpu().numpy().tobytes() == counts.tobytes() and loc.sums.cpu().numpy().tobytes() == sums.tobytes()
    with pytest.raises(ValueError):
        loc.update(c1["gt_count"], c1["gt_positions"], c1["gt_boxes"], k=case["B"] + 1)
    with pytest.raises(ValueError):
        loc.update(c1["gt_count"], c1["gt_positions"][:, :1], c1["gt_boxes"])
    with pytest.raises(ValueError):
        loc.update(_dev(c1["gt_count"]).long(), c1["gt_positions"], c1["gt_boxes"])


def test_module_on_a_real_model_and_a_scene_source(H):
    """AIRModel(cnn=False, train=False) at B = 8, T = 3 on scenes a DeviceSceneSource composed into its input buffer;
    source.meta() goes straight in.  Accumulators and values() equal the restatement on the model's records copied to the
    host.  (The z_pres bias of a fresh model is raised until it infers objects: the scores then have something to sum.)"""
    import multi_mnist as mm
    from air import air_model as am
    from air.metrics import Localization
    from oracle import air_oracle as ao
    hp = dict(ao.TRAINING_HP)
    B, T, G = 8, hp["max_steps"], 2
    assert T == 3
    am.reset_default_graph()
    images = torch.zeros(B, hp["canvas_size"] ** 2, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    model = am.AIRModel(images, digits, cnn=False, train=False, scope="loc8", gemm_precision="fp32", **hp)
    params = {k: np.array(v) for k, v in ao.init_params(hp, 0).items()}
    bias = "z_pres/log_odds/output/biases"
    source = mm.DeviceSceneSource(mm.load_glyphs()[0], B, images, digits, canvas_dim=hp["canvas_size"], max_digits=G, seed=5)
    source.next_batch()
    for raised in range(12):
        model.load_state_dict(params)
        model.forward()
        if int(model.run_digits.sum()) >= 4:
            break
        params[bias] = params[bias] + np.float32(1.0)
    print("z_pres bias raised %d times: inferred counts %s" % (raised, model.run_digits.tolist()))
    loc = Localization(model, G, per_digit=True)
    meta = source.meta()
    assert tuple(meta["positions"].shape) == (B, 2 * G)
    loc.update(digits, meta["positions"], meta["boxes"])
    values = loc.values()
    case = dict(T=T, B=B, G=G, canvas_size=hp["canvas_size"], tau=0.5)
    chunk = dict(k=B, att=model.att.cpu().numpy(), run_digits=model.run_digits.cpu().numpy(), gt_count=digits.cpu().numpy(),
                 gt_positions=meta["positions"].cpu().numpy().reshape(B, G, 2), gt_boxes=meta["boxes"].cpu().numpy().reshape(B, G, 2))
    counts, sums = lc.empty_accumulators(case)
    match, iou = lc.apply_chunk(case, chunk, counts, sums)
    print("real model: counts %s sums %s" % (counts[:lc.COUNTS].tolist(), sums.tolist()))
    assert counts[lc.PRESENT] > 0 and counts[lc.INFERRED] > 0
    assert loc.counts.cpu().numpy().tobytes() == counts.tobytes() and loc.sums.cpu().numpy().tobytes() == sums.tobytes()
    assert loc.match.cpu().numpy().tobytes() == match.tobytes() and loc.iou.cpu().numpy().tobytes() == iou.tobytes()
    assert values.cpu().numpy().tobytes() == lc.derived(counts, sums).tobytes()
    # the [k, G, 2] form of the same tensors agrees
    again = Localization(model, G)
    again.update(digits, meta["positions"].view(B, G, 2), meta["boxes"].view(B, G, 2))
    assert torch.equal(again.counts, loc.counts) and torch.equal(again.sums, loc.sums)
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        Localization(model, G).update(digits, meta["positions"].cpu(), meta["boxes"])
