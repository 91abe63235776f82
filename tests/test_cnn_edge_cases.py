"""CPU-side checks of tests/cnn_edge_cases.py: everything tests/test_gpu_cnn_edges.py takes for granted about its inputs and
its reference is asserted here, from the float64 reference alone.

  * the Python restatement of cnn_lds answers as the library's host-side check does (air_cnn_workspace_floats, no GPU) at
    every (S, F), so it reproduces tests/test_cnn_abi.py's last-canvas table; the case table takes both sides of both
    max() choices of the layout and holds the canvases on either side of the "compact + codes" switch at F = 8;
  * exact-integer cases: the inputs come from their value sets, every chain's sum of |term| is below 2^24, every reference
    tensor is exactly representable in fp32, every compared tensor holds a non-zero, from S = 13 up every case holds sites
    at which `>=` in place of `>` would move a gradient (three masks, two pools), and the seed is the first that does all this;
  * real-valued cases: the margins of tests/test_gpu_cnn.py's precondition, at the first seed that meets them; the
    forward-only cases at the first seed with a live output;
  * the numpy reference against torch (relu, max_pool2d, autograd, float64) on a tie-heavy case: the same codes, the same
    gradients, and torch.clamp(min=0) -- which passes a gradient at an exact zero -- is shown to differ."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import abi_check as abi
import cnn_edge_cases as E

ids = lambda c: "B%d-S%d-F%d" % c  # noqa: E731


@pytest.fixture(scope="module")
def H():
    return abi.hip()


def test_lds_restatement_answers_as_the_library(H):
    ws = H.lib().air_cnn_workspace_floats
    for F in range(0, 10):
        for S in range(3, 131):
            rc = E.served(S, F)
            assert ws(3, S, F) == (3 * E.num_partials(F) if rc == 0 else rc), (S, F)
    for F, S in E.LAST_CANVAS.items():
        assert E.served(S, F) == 0 and E.served(S + 1, F) == -2, (F, S)
        assert (2, S, F) in E.LIMITS and (2, S, F) in E.EXACT_CASES and (2, S, F) in E.REAL_FORWARD_CASES
    # how close the last canvases sit to the grant: 163 136 of 163 840 bytes at (77, 8)
    assert E.cnn_lds(77, 8)["bytes"] == 163136
    assert all(E.cnn_lds(S, F)["bytes"] > 0.96 * E.LDS_LIMIT for F, S in E.LAST_CANVAS.items() if F > 2)


def test_sq_partials_count(H):
    n = H.lib().air_cnn_num_sq_partials
    for F in range(1, 9):
        assert n(F) == E.num_sq_partials(F) == -(-(25 * F + 50 * F * F + 3 * F) // 256)
    assert [E.num_sq_partials(F) for F in (1, 8)] == [1, 14]
    assert sorted(E.num_partials(F) % 256 for F in range(1, 9)) == [0, 22, 78, 86, 96, 110, 144, 176]   # full at F = 2, else ragged


def test_case_table_takes_every_layout_branch():
    for table in (E.EXACT_CASES, E.REAL_FORWARD_CASES):
        assert {E.cnn_lds(S, F)["r1_is"] for _, S, F in table} == {"g3h|p2h", "image"}
        assert {E.cnn_lds(S, F)["r4_is"] for _, S, F in table} == {"compact+codes", "haloed"}
    side = lambda S: E.cnn_lds(S, 8)["r4_is"]  # noqa: E731
    assert [S for S in range(4, 78) if side(S) == "compact+codes"] == [68, 69, 72, 73, 76, 77]
    assert side(77) == side(69) == side(68) == "compact+codes" and side(70) == side(67) == "haloed"
    for S in (69, 68, 70, 67):
        assert (2, S, 8) in E.COMPACT_EDGE and (2, S, 8) in E.EXACT_CASES
    # by how little: 8 floats at S1 = 34 -- an overlay one row short would corrupt the code bytes
    L = E.cnn_lds(68, 8)
    assert L["b_total"] - L["b_r4"] - E.r4(8 * L["pl1"]) == 8
    # the overlays the kernels rely on, at every served size: what is written into a region fits it
    for F in range(1, 9):
        for S in range(4, 129):
            if E.served(S, F):
                continue
            L = E.cnn_lds(S, F)
            r1, r4n = L["b_r2"] - L["b_r1"], L["b_total"] - L["b_r4"]
            assert r1 >= L["IP"] * (S + 4) and r1 >= E.r4(F * L["pl2"]) + F * L["pl2"]
            assert r4n >= F * L["pl1"] and 4 * (L["b_total"] - L["b_code"]) >= F * L["S1"] ** 2 and L["b_code"] - L["b_r4"] >= F * L["S1"] ** 2


def test_case_table_holds_what_the_issue_names():
    assert sorted(F for _, S, F in E.INSTANTIATION_EXACT) == list(range(1, 9))
    assert sorted(F for _, S, F in E.INSTANTIATION_REAL) == [1, 2, 4, 6, 7]
    assert {(S, F) for _, S, F in E.SMALLEST} == {(S, F) for S in (4, 5, 6, 7) for F in (1, 8)}
    assert {B for B, _, _ in E.SMALLEST} == {1, 2} and len(E.SMALLEST) == 16
    assert all(S // 4 == 1 for _, S, _ in E.SMALLEST)
    S1 = {S: S // 2 for _, S, _ in E.THREAD_EDGES}
    assert S1[32] ** 2 == E.FWD_NT and S1[34] ** 2 == E.FWD_NT + 33
    assert 22 * 22 < E.BWD_NT < 23 * 23
    assert [b - 1 for b in E.BATCH_SIZES] == [0, 1, 7, 8, 9, 16]
    assert all(c in E.EXACT_CASES for c in E.OPTIONAL_CASES)
    assert len(set(E.EXACT_CASES)) == len(E.EXACT_CASES)


@pytest.mark.parametrize("case", E.EXACT_CASES, ids=ids)
def test_exact_case_conditions(case):
    B, S, F = case
    P, images, d_out, ref = E.exact_case(*case)
    assert set(np.unique(images)) <= {0.0, 1.0, 2.0, 3.0} and set(np.unique(d_out)) <= {-1.0, 0.0, 1.0}
    for n in E.NAMES:
        assert set(np.unique(P[n])) <= {-1.0, 0.0, 1.0} and P[n].dtype == np.float32
    assert images.shape == (B, S * S) and d_out.shape == (B, (S // 4) ** 2 * F)
    # any accumulation order is exact: integers, and every chain's sum of |term| below 2^24
    worst = max(ref["bounds"], key=ref["bounds"].get)
    assert ref["bounds"][worst] < E.EXACT_LIMIT, (worst, ref["bounds"][worst])
    for n in E.COMPARED + ["partials"]:
        a = ref[n]
        assert np.array_equal(a, np.round(a)) and np.array_equal(a.astype(np.float32).astype(np.float64), a), n
    for n in E.COMPARED:
        assert np.any(ref[n] != 0), n
    assert ref["arg1"].max() <= 3 and ref["arg2"].max() <= 3
    assert np.array_equal(ref["partials"].sum(axis=0), np.concatenate([ref[n].reshape(-1) for n in E.NAMES]))
    if S >= 13:
        assert min(ref["bites"].values()) > 0, ref["bites"]
        assert ref["zeros"] > 0
    # the seed is the first that meets the conditions
    for seed in range(E.exact_seed(*case)):
        assert not E.exact_ok(E.reference(*E._exact_inputs(seed, *case))), seed


def test_exact_limit_cases_stay_far_below_2_to_the_24():
    worst = max(max(E.exact_case(*c)[3]["bounds"].values()) for c in E.LIMITS)
    print("largest sum of |term| at the last canvases: %.4g (%.2f %% of 2^24)" % (worst, 100 * worst / E.EXACT_LIMIT))
    assert worst <= 0.01 * E.EXACT_LIMIT


@pytest.mark.parametrize("case", E.INSTANTIATION_REAL + [(E.BATCH_MAX, E.BATCH_S, E.BATCH_F)], ids=ids)
def test_real_case_meets_the_precondition_at_its_first_seed(case):
    seed = E.real_seed(*case)
    P, images, d_out, ref = E.real_case(*case)
    assert ref["relu_margin"] >= E.MARGIN and ref["pool_margin"] >= E.MARGIN
    for s in range(1, seed):
        assert not E.margins_ok(E.reference(*E._real_inputs(s, *case))), s
    assert all(np.any(ref[n] != 0) for n in E.COMPARED)


def test_batch_cases_are_prefixes_of_one_draw():
    P17, im17, d17, ref17 = E.batch_case(E.BATCH_MAX)
    for B in E.BATCH_SIZES:
        P, images, d_out, ref = E.batch_case(B)
        assert np.array_equal(images, im17[:B]) and np.array_equal(d_out, d17[:B])
        assert all(np.array_equal(P[n], P17[n]) for n in E.NAMES)
        assert np.array_equal(ref["partials"], ref17["partials"][:B])          # an image's gradients do not depend on the batch
        assert E.margins_ok(ref)
    import test_gpu_cnn as T                                                    # the recipe is that file's
    for n in E.NAMES:
        assert np.array_equal(T._variables(7, 5)[n], E.variables(7, 5)[n])
    assert E.MARGIN == T.MARGIN


@pytest.mark.parametrize("case", E.REAL_FORWARD_CASES, ids=ids)
def test_forward_only_case_is_live_at_its_first_seed(case):
    P, images, ref = E.real_forward_case(*case)
    assert E.live_ok(ref)
    for s in range(1, E.real_forward_seed(*case)):
        Ps, ims, _ = E._real_inputs(s, *case)
        assert not E.live_ok(E.reference(Ps, ims)), s


def _torch_block(P, images, d_out, S, act):
    x = torch.tensor(images, dtype=torch.float64).view(-1, 1, S, S).requires_grad_(True)
    V = [torch.tensor(P[n], dtype=torch.float64, requires_grad=True) for n in E.NAMES]
    conv = lambda h, k, b: TF.conv2d(h, k.permute(3, 2, 0, 1), b, padding=2)  # noqa: E731
    r1 = act(conv(x, V[0], V[1])); p1, i1 = TF.max_pool2d(r1, 2, 2, return_indices=True)
    r2 = act(conv(p1, V[2], V[3])); p2, i2 = TF.max_pool2d(r2, 2, 2, return_indices=True)
    out = act(conv(p2, V[4], V[5])).permute(0, 2, 3, 1).reshape(x.shape[0], -1)
    grads = torch.autograd.grad((out * torch.tensor(d_out, dtype=torch.float64)).sum(), [x] + V)

    def codes(idx, width):
        n = idx.shape[-1]
        wy, wx = torch.arange(n).view(1, 1, n, 1), torch.arange(n).view(1, 1, 1, n)
        return (2 * (idx // width - 2 * wy) + (idx % width - 2 * wx)).permute(0, 2, 3, 1).numpy().astype(np.uint8)
    return dict(out=out.detach().numpy(), pool1=p1.detach().permute(0, 2, 3, 1).numpy(), pool2=p2.detach().permute(0, 2, 3, 1).numpy(),
                arg1=codes(i1, S), arg2=codes(i2, S // 2), d_images=grads[0].numpy().reshape(x.shape[0], -1),
                **{n: g.numpy() for n, g in zip(E.NAMES, grads[1:])})


def test_numpy_reference_is_torch_relu_and_max_pool_on_ties():
    case = (2, 34, 4)
    P, images, d_out, ref = E.exact_case(*case)
    assert min(ref["bites"].values()) >= 9                      # tie-heavy, zero-heavy
    got = _torch_block(P, images, d_out, case[1], torch.relu)
    for n in ["out", "pool1", "pool2", "arg1", "arg2", "d_images"] + E.NAMES:
        assert np.array_equal(got[n], ref[n]), n
    # clamp(min=0) passes the gradient at an exact zero: not this block's rule
    other = _torch_block(P, images, d_out, case[1], lambda t: t.clamp(min=0.0))
    assert np.array_equal(other["out"], ref["out"])
    assert any(not np.array_equal(other[n], ref[n]) for n in E.NAMES)
    # and on a real-valued case, where nothing is exact: the same routing, the same numbers to float64 rounding
    P, images, d_out, ref = E.real_case(3, 13, 6)
    got = _torch_block(P, images, d_out, 13, torch.relu)
    assert np.array_equal(got["arg1"], ref["arg1"]) and np.array_equal(got["arg2"], ref["arg2"])
    for n in ["out", "d_images"] + E.NAMES:
        assert np.abs(got[n] - ref[n]).max() <= 1e-12 * np.abs(ref[n]).max(), n


def test_sq_slices():
    g = [np.arange(300, dtype=np.float64), np.ones(5)]
    s = E.sq_slices(g)
    assert s.shape == (2,) and s[0] == np.square(np.arange(256.0)).sum() and s[1] == np.square(np.arange(256.0, 300.0)).sum() + 5
