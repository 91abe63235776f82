"""GPU tests of the latent probe (air_latent_probe of include/air_hip.h, air.metrics.LatentProbe, air.embeddings.probe).

The reference is the float64 restatement of tests/latent_probe_cases.py.  Everything is compared BIT FOR BIT: the int64
counts, pred, neighbours, and the fp64 neighbour_d2 and moments as bit patterns -- the arithmetic and its order are fully
stated, so there is no tolerance.  Inputs and outputs sit between guard bands (NaN around the codes, sentinels around
everything else) that must be intact afterwards, and rows >= M_eff of the codes are NaN: reading one would show."""
import ctypes as C

import numpy as np
import pytest
import torch

import abi_check as abi
import latent_probe_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 8                                    # sentinel elements in front of and behind every buffer
FILL_I32, FILL_I64, FILL_F64 = -5, -(2 ** 40) - 5, -7.25
CASES = pc.cases()
KEYS = ("pred", "neighbours", "neighbour_d2", "counts", "moments")


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
        for band in (host[:GUARD], host[GUARD + self.n:]):
            assert np.isnan(band).all() if self.fill != self.fill else (band == self.fill).all(), "a sentinel was overwritten"
        return host[GUARD:GUARD + self.n]


def run_case(H, case, per_row=True):
    """one air_latent_probe call -> the five outputs as numpy (the per-row ones only with per_row); every output starts as
    sentinels, so an element the call does not write shows"""
    x, labels, k, classes = case["x"], case["labels"], case["k"], case["classes"]
    M, Z = x.shape
    lat = Guarded(M * Z, torch.float32, float("nan"), init=_dev(x.reshape(-1)))
    lab = Guarded(M, torch.int32, FILL_I32, init=_dev(labels))
    rows = None if case["rows"] is None else torch.tensor([case["rows"]], dtype=torch.int32, device="cuda")
    nbytes = H.lib().air_latent_probe_workspace_bytes(M, Z, k)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = Guarded(nbytes // 8, torch.float64, FILL_F64)
    out = dict(pred=Guarded(M, torch.int32, FILL_I32), neighbours=Guarded(M * k, torch.int32, FILL_I32),
               neighbour_d2=Guarded(M * k, torch.float64, FILL_F64),
               counts=Guarded(pc.COUNTS + classes * classes, torch.int64, FILL_I64), moments=Guarded(2 * Z, torch.float64, FILL_F64))
    opt = (lambda key: H.ptr(out[key].view)) if per_row else (lambda key: None)
    a = H.LatentProbe(H.ptr(lat.view), H.ptr(lab.view), H.ptr(rows), opt("pred"), opt("neighbours"), opt("neighbour_d2"),
                      H.ptr(out["counts"].view), H.ptr(out["moments"].view), M, Z, k, classes, case["au_threshold"])
    H.launch("air_latent_probe", torch.device("cuda"), C.byref(a), H.ptr(ws.view))
    torch.cuda.synchronize()
    ws.payload(), lat.payload(), lab.payload()
    got = {key: g.payload() for key, g in out.items()}
    if not per_row:
        assert (got["pred"] == FILL_I32).all() and (got["neighbours"] == FILL_I32).all() and (got["neighbour_d2"] == FILL_F64).all()
    got["neighbours"], got["neighbour_d2"] = got["neighbours"].reshape(M, k), got["neighbour_d2"].reshape(M, k)
    return got


def check_case(H, name):
    want, got = pc.expected(name), run_case(H, CASES[name])
    print("%s: counts %s" % (name, got["counts"][:pc.COUNTS].tolist()))
    assert pc.same_bits(want, got) == [], (name, got["counts"][:pc.COUNTS], want["counts"][:pc.COUNTS])
    return got


@pytest.mark.parametrize("name", [pc.shape_name(s) for s in pc.SHAPES])
def test_kernel_equals_the_restatement(H, name):
    """(M, Z, k, classes): M = 1, 2, k, k + 1, around the query tile (64), the reference tile (32) and one row beyond the
    full set of splits (257, where a run holds two tiles and the last runs none); Z = 1, 2, 50, 51, 256 (the last beyond 48
    KB of LDS); k = 1, 5, 16 (both list widths); 1, 2, 10 and 64 classes"""
    check_case(H, name)


def test_ties_go_to_the_smaller_row_and_the_earlier_class(H):
    """codes on a half-integer grid: 116 of 130 queries tie at the k-th neighbour, 63 of them across reference tiles and
    splits, and 41 rows share their top vote -- tests/test_latent_probe_cases.py asserts the inputs do"""
    check_case(H, "ties")


def test_duplicates_and_the_case_without_ties(H):
    got = check_case(H, "duplicates")
    assert (got["neighbour_d2"][:12, 0] == 0.0).all() and got["neighbours"][:12, 0].tolist() == list(range(28, 40))
    check_case(H, "gaussian")


@pytest.mark.parametrize("name", pc.VALIDITY)
def test_invalid_rows_are_neither_queries_nor_neighbours(H, name):
    """a NaN row, two Inf rows, a label of -1, a label equal to classes, every row invalid (V = 0: NaN moments), exactly one
    valid row (nothing to compare it with)"""
    got = check_case(H, name)
    at = CASES[name]["planted"][name]
    assert got["pred"][at] == -1 and (got["neighbours"][at] == -1).all()


@pytest.mark.parametrize("name", sorted(pc.ROWS_CASES))
def test_the_rows_pointer_is_clamped_and_hides_the_rest(H, name):
    """*rows = 0, < M, > M and negative (the null pointer: every other case); rows >= M_eff are NaN"""
    got = check_case(H, name)
    assert got["counts"][pc.ROWS] == min(max(pc.ROWS_CASES[name], 0), 70)


@pytest.mark.parametrize("name", ["ties", "m257_z3_k5_c10", "nan_row", "m17_z256_k16_c64"])
def test_without_the_optional_outputs_the_counts_are_the_same(H, name):
    want, got = pc.expected(name), run_case(H, CASES[name], per_row=False)
    assert got["counts"].tobytes() == want["counts"].tobytes() and got["moments"].tobytes() == want["moments"].tobytes()


def test_the_same_inputs_give_the_same_bits(H):
    a, b = run_case(H, CASES["ties"]), run_case(H, CASES["ties"])
    assert pc.same_bits(a, b) == []


# -------------------------------------------------------------------------------------------------------------- the module
CANVAS, WINDOW = 50, 4


class _Pass:
    """what LatentProbe reads of a model; chunk() leaves the records of a pass that found the digits of the ground truth"""

    def __init__(self, T, B, Z):
        self.max_steps, self.batch_size, self.canvas_size, self.windows_size, self.vae_latent_dimensions = T, B, CANVAS, WINDOW, Z
        self.input_images = torch.zeros(B, CANVAS ** 2, device="cuda")
        self.ensured = 0

    def _ensure(self):
        self.ensured += 1


def _chunk(model, G, counts, found, codes, labels):
    """images with counts[i] digits side by side; the pass inferred found[i] of them, exactly at their centres, with
    `codes` as the latent means of the matched ones in (image, digit) order -> the ground truth, the rows used"""
    T, B, Z = model.max_steps, model.batch_size, model.vae_latent_dimensions
    k = len(counts)
    att = np.zeros((T, B, 16), np.float32)
    ml = np.full((T, B, 2 * Z), 9.5, np.float32)
    pos, box, lab = np.zeros((k, G, 2), np.int32), np.zeros((k, G, 2), np.int32), np.full((k, G), 3, np.int32)
    row = 0
    for i in range(k):
        for g in range(counts[i]):
            pos[i, g], box[i, g] = (5 + 20 * g, 7), (10, 12)
            if g < found[i]:
                att[g, i, 1] = ((5 + 20 * g) * 2 + 10 - 1.0) / 2.0 / ((CANVAS - 1) / 2.0) - 1.0
                att[g, i, 2] = (7 * 2 + 12 - 1.0) / 2.0 / ((CANVAS - 1) / 2.0) - 1.0
                ml[g, i, :Z], lab[i, g] = codes[row], labels[row]
                row += 1
    run = np.zeros(B, np.int32)
    run[:k] = found
    model.att, model.ml, model.run_digits = _dev(att), _dev(ml), _dev(run)
    model.vrec = torch.zeros(T, B, WINDOW * WINDOW, device="cuda")
    return (np.asarray(counts, np.int32), pos, box, lab), row


def _padded(case, lo, hi, capacity):
    x = np.zeros((capacity, case["x"].shape[1]), np.float32)
    labels = np.zeros(capacity, np.int32)
    x[:hi - lo], labels[:hi - lo] = case["x"][lo:hi], case["labels"][lo:hi]
    return x, labels


def test_module_collects_scores_resets_and_reports_an_overflow(H):
    """two update() chunks (device tensors, then numpy arrays in the [k, 2 G] layout), then score(): the restatement on the
    concatenated rows; values() and result(); reset(); a store too small"""
    from air.metrics import LatentProbe
    case = CASES["duplicates"]
    x, labels, k, classes = case["x"], case["labels"], case["k"], case["classes"]
    G, B, cap = 2, 16, 48
    model = _Pass(3, B, x.shape[1])
    probe = LatentProbe(model, G, classes=classes, k=k, capacity=cap, per_row=True)
    assert probe.names() == list(pc.NAMES)
    counts0, found0 = [2] * 8 + [1] * 6 + [1, 0], [2] * 8 + [1] * 6 + [0, 0]          # image 14: a digit nothing was inferred for
    truth0, n0 = _chunk(model, G, counts0, found0, x, labels)
    assert n0 == 22
    probe.update(*(_dev(t) for t in truth0))
    counts1 = [2] * 6 + [1] * 6                                                       # 12 images of the 16 batch rows
    truth1, n1 = _chunk(model, G, counts1, counts1, x[n0:], labels[n0:])
    assert n0 + n1 == len(x) == 40
    probe.update(truth1[0], truth1[1].reshape(12, 2 * G), truth1[2].reshape(12, 2 * G), truth1[3])
    probe.score()
    values = probe.values()
    assert model.ensured == 2 and values.is_cuda and values.dtype == torch.float64
    assert probe.counters.tolist() == [40, 41, 40, 0]
    want = pc.probe(*_padded(case, 0, 40, cap), k, classes, rows=40)
    got = {key: getattr(probe, key).cpu().numpy() for key in KEYS}
    assert pc.same_bits(want, got) == []
    assert probe.latents[:40].cpu().numpy().tobytes() == x.tobytes() and probe.labels[:40].cpu().numpy().tobytes() == labels.tobytes()
    assert values.cpu().numpy().tobytes() == pc.derived(want["counts"], 40, 41).tobytes()
    into = torch.zeros(len(pc.NAMES), dtype=torch.float64, device="cuda")
    assert probe.values(into) is into and torch.equal(into, values)
    assert probe.confusion().cpu().numpy().tobytes() == pc.confusion(want["counts"], classes).tobytes()
    res = probe.result()
    assert [res[n] for n in pc.NAMES] == pc.derived(want["counts"], 40, 41).tolist()
    assert res["confusion"].tobytes() == pc.confusion(want["counts"], classes).tobytes() and not res["overflow"]
    assert (res["matched"], res["present"], res["rows"], res["valid"]) == (40, 41, 40, 40)
    assert res["mean"].tobytes() == want["moments"][:x.shape[1]].tobytes() and res["variance"].tobytes() == want["moments"][x.shape[1]:].tobytes()
    conf = pc.confusion(want["counts"], classes)
    assert np.array_equal(res["recall"], np.diag(conf) / conf.sum(axis=1))
    # reset(): the second chunk alone
    probe.reset()
    assert probe.counters.tolist() == [0, 0, 0, 0] and np.isnan(probe.values().cpu().numpy()[[0, 3]]).all()
    probe.update(*truth1)
    probe.score()
    want = pc.probe(*_padded(case, n0, 40, cap), k, classes, rows=n1)
    assert pc.same_bits(want, {key: getattr(probe, key).cpu().numpy() for key in KEYS}) == []
    # a store of 30 rows: the first 30 are scored, the overflow is reported
    small = LatentProbe(model, G, classes=classes, k=k, capacity=30)
    assert small.pred is None
    _chunk(model, G, counts0, found0, x, labels)
    small.update(*truth0)
    _chunk(model, G, counts1, counts1, x[n0:], labels[n0:])
    small.update(*truth1)
    small.score()
    res = small.result()
    want = pc.probe(x[:30], labels[:30], k, classes)
    assert res["overflow"] and res["matched"] == 40 and res["rows"] == 30
    assert small.counts.cpu().numpy().tobytes() == want["counts"].tobytes() and small.moments.cpu().numpy().tobytes() == want["moments"].tobytes()
    with pytest.raises(ValueError):
        probe.update(*truth1, k=B + 1)
    with pytest.raises(ValueError):
        probe.update(truth1[0], truth1[1], truth1[2], truth1[3][:, :1])
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        probe.update(_dev(truth1[0]).cpu(), *truth1[1:])


def test_module_on_a_real_model_and_a_scene_source(H):
    """AIRModel(cnn=False, train=False) at B = 8, T = 3 on scenes a DeviceSceneSource composed into its input buffer, the
    labels of its glyphs as the classes.  The collected latents are read back and the restatement run on them.  (The z_pres
    bias of a fresh model is raised until it infers objects, as tests/test_gpu_localization.py does; the match is the
    projector export's, so max_distance is opened wide enough that at least 4 of the inferred objects take a digit.)"""
    import multi_mnist as mm
    from air import air_model as am
    from air.metrics import LatentProbe
    from oracle import air_oracle as ao
    hp = dict(ao.TRAINING_HP)
    B, T, G = 8, hp["max_steps"], 2
    am.reset_default_graph()
    images = torch.zeros(B, hp["canvas_size"] ** 2, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    model = am.AIRModel(images, digits, cnn=False, train=False, scope="probe8", gemm_precision="fp32", **hp)
    params = {k: np.array(v) for k, v in ao.init_params(hp, 0).items()}
    bias = "z_pres/log_odds/output/biases"
    glyphs, glyph_labels, _ = mm.load_glyphs()
    source = mm.DeviceSceneSource(glyphs, B, images, digits, canvas_dim=hp["canvas_size"], max_digits=G, seed=5)
    source.next_batch()
    for raised in range(12):
        model.load_state_dict(params)
        model.forward()
        if bool((model.run_digits > 0).all()):                   # every image has an object a digit can take
            break
        params[bias] = params[bias] + np.float32(1.0)
    meta = source.meta()
    labels = torch.from_numpy(np.asarray(glyph_labels, np.int32)).cuda()[meta["indices"].long().clamp(min=0)].contiguous()
    probe = LatentProbe(model, G, k=3, per_row=True, max_distance=2.9)
    probe.update(digits, meta["positions"], meta["boxes"], labels)
    probe.score()
    values = probe.values()
    matched, present, inferred, overflow = probe.counters.tolist()
    print("z_pres bias raised %d times: inferred counts %s, %d of %d digits matched" % (raised, model.run_digits.tolist(), matched, present))
    assert matched >= 4 and not overflow and inferred == int(model.run_digits.sum())
    Z = hp["vae_latent_dimensions"]
    x, lab = probe.latents.cpu().numpy(), probe.labels.cpu().numpy()
    # the rows are the posterior means of the matched objects: every collected row is a row of the model's ml
    means = model.ml[:, :, :Z].reshape(-1, Z).cpu().numpy()
    assert all((means == x[r]).all(axis=1).any() for r in range(matched))
    want = pc.probe(x, lab, 3, 10, rows=matched)
    print("real model: counts %s" % want["counts"][:pc.COUNTS].tolist())
    assert want["counts"][pc.SCORED] == matched
    assert pc.same_bits(want, {key: getattr(probe, key).cpu().numpy() for key in KEYS}) == []
    assert values.cpu().numpy().tobytes() == pc.derived(want["counts"], matched, present).tobytes()
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        probe.update(digits, meta["positions"].cpu(), meta["boxes"], labels)


def test_embeddings_probe_on_tensors(H):
    from air import embeddings
    case = CASES["gaussian"]
    M = len(case["x"])
    result = embeddings.Embeddings(_dev(case["x"]), torch.zeros(M, 4, 4, device="cuda"), _dev(case["labels"]),
                                   torch.arange(M, dtype=torch.int32, device="cuda"), M, M, M)
    got, want = embeddings.probe(result, k=case["k"], classes=case["classes"]), pc.expected("gaussian")
    Z = case["x"].shape[1]
    assert got["confusion"].tobytes() == pc.confusion(want["counts"], case["classes"]).tobytes()
    assert (got["scored"], got["correct"], got["active_units"], got["rows"], got["valid"]) == tuple(
        int(want["counts"][i]) for i in (pc.SCORED, pc.CORRECT, pc.ACTIVE_UNITS, pc.ROWS, pc.VALID))
    assert got["knn_accuracy"] == want["counts"][pc.CORRECT] / want["counts"][pc.SCORED]
    assert got["mean"].tobytes() == want["moments"][:Z].tobytes() and got["variance"].tobytes() == want["moments"][Z:].tobytes()
    with pytest.raises(ValueError, match="nothing to probe"):
        embeddings.probe(embeddings.Embeddings(result.latents[:0], result.windows[:0], result.labels[:0], result.ids[:0], M, M, 0))
    with pytest.raises(H.AirHipError, match="no CPU fallback"):
        embeddings.probe(embeddings.Embeddings(result.latents.cpu(), result.windows, result.labels, result.ids, M, M, M))
