"""CPU: the case tables, references and input conditions of tests/around_step_cases.py, which tests/test_gpu_around_step.py
runs on the device -- the tables reach the edges they name, the references are right on cases small enough to state by hand,
every condition placed on the inputs holds (computed from the float64 reference alone), and the kernel's expressions in
numpy fp32 lie within a quarter of each bound."""
import numpy as np

import around_step_cases as asc
import pointwise_edge_cases as pec
import step_limit_cases as slc
from air import _hip as H
from oracle import shuffle_queue as sq
from oracle import summaries as osum


# ---- 1. the shuffle queue ---------------------------------------------------------------------------------------------
def test_queue_geometries_reach_both_resolvers_and_the_limits():
    G = asc.QUEUE_GEOMETRIES
    assert len(G) == len(set(G)) == 9
    for cap, batch, mad, n_rec in G + [asc.LARGE_GEOMETRY]:
        assert batch % 4 == 0 and 0 < batch <= 1024 and cap - batch >= mad >= 0 and n_rec > 0
        assert cap * 4 + batch * 8 <= asc.LDS_LIMIT
    at_limit = [g for g in G if g[0] * 4 + g[1] * 8 == asc.LDS_LIMIT]
    assert sorted(g[1] for g in at_limit) == [64, 1024]                        # the reference's batch and the largest one
    assert sum(g[1] > asc.WAVE for g in G) >= 5 and sum(g[1] <= asc.WAVE for g in G) >= 4
    assert any(g[1] == asc.WAVE + 4 for g in G) and any(g[1] == asc.WAVE for g in G)   # the two sides of the branch
    assert any(g[0] == g[1] for g in G)                                         # every slot a back
    assert any(g[3] == 1 for g in G) and any(g[3] < g[1] for g in G) and any(g[3] > g[0] for g in G)
    assert any(g[1] == 4 and g[0] > 4 for g in G)                               # one drawing thread
    assert asc.schedule_batches(asc.QUEUE_SCHEDULE) == 20 and asc.QUEUE_SCHEDULE[1] == ("many", 5)
    # the large state: the four single dequeues cross the wrap of the counter's low word, and pos mod n_records needs 64 bits
    (pos, n), nb = asc.LARGE_STATE, asc.schedule_batches(asc.LARGE_SCHEDULE)
    assert n < 2 ** 32 <= n + asc.LARGE_SCHEDULE[0][1] - 1 and pos >= 2 ** 32 and nb == 7
    assert pos % asc.LARGE_GEOMETRY[3] != (pos & 0xFFFFFFFF) % asc.LARGE_GEOMETRY[3]
    q = asc.large_state_queue()
    assert len(q) == asc.LARGE_GEOMETRY[0] and 0 <= min(q) and max(q) < asc.LARGE_GEOMETRY[3] and len(set(q)) < len(q)
    assert sq.device_draws(asc.LARGE_SEED, 2 ** 32, 8) != sq.device_draws(asc.LARGE_SEED, 0, 8)      # the high word is in the counter


def test_literal_dequeue_is_the_batch_level_model():
    """the single dequeue from a given state, chained from (capacity, 0), is tf_queue_batches; and it starts anywhere"""
    for geometry in [(100, 8, 50, 37), (68, 64, 0, 7), (4, 4, 0, 1), (128, 128, 0, 50)]:
        cap, batch, mad, n_rec = geometry
        picks, q, state = asc.queue_model(geometry, 9, (("single", 6),))
        ref = sq.tf_queue_batches(n_rec, cap, batch, mad, 6, lambda n, k: sq.device_draws(9, n, k))
        assert np.array_equal(picks, ref) and state == (cap + 6 * batch, 6)
        assert sorted(q[cap - batch:]) == sorted((cap + 5 * batch + t) % n_rec for t in range(batch))
    # by hand: draws 5, 0, 7, 2 on the queue 10 .. 15 with the stream at 100 of 1000
    picks, new = sq.literal_dequeue([10, 11, 12, 13, 14, 15], 4, [5, 0, 7, 2], 100, 1000)
    #  5 % 6 = 5 -> 15, back 15 into 5;  0 % 5 = 0 -> 10, back 14 into 0;  7 % 4 = 3 -> 13, back 13;  2 % 3 = 2 -> 12, back 12
    assert picks == [15, 10, 13, 12] and new == [14, 11, 100, 101, 102, 103]
    # the large state continues from where it is put
    start = (asc.LARGE_STATE, tuple(asc.large_state_queue()))
    picks, q, state = asc.queue_model(asc.LARGE_GEOMETRY, asc.LARGE_SEED, asc.LARGE_SCHEDULE, start)
    assert state == (asc.LARGE_STATE[0] + 7 * 8, asc.LARGE_STATE[1] + 7) and picks.shape == (7, 8)
    assert list(q[-8:]) == [(asc.LARGE_STATE[0] + 6 * 8 + t) % 37 for t in range(8)]


def test_parallel_dequeue_is_the_literal_queue_past_one_wave():
    """the rule of the generic resolver (64 < batch <= 1024) against the literal dequeue: batches 68, 128, 256 and 1024,
    capacity == batch among them, random draws and draws in 0 .. 4 that collide all the time"""
    rng = np.random.RandomState(1)
    for batch, trials in ((68, 12), (128, 8), (256, 4), (1024, 2)):
        for trial in range(trials):
            cap = batch if trial % 2 == 0 else batch + int(rng.randint(1, 3 * batch))
            n_rec = 997
            q = [int(v) for v in rng.permutation(cap + 1000)[:cap]]
            pos = int(rng.randint(0, 1000))
            for kind in ("random", "colliding"):
                r = [int(v) for v in (rng.randint(0, 2 ** 32, size=batch, dtype=np.uint64) if kind == "random" else rng.randint(0, 5, size=batch))]
                want = sq.literal_dequeue(q, batch, r, pos, n_rec)
                got = sq.parallel_dequeue(q, batch, r, pos, n_rec)
                assert got[0] == want[0] and got[1] == want[1], (batch, cap, kind)
                q, pos = want[1], pos + batch
    # every geometry of the device test, through the device's own draws
    for geometry in asc.QUEUE_GEOMETRIES:
        cap, batch, _, n_rec = geometry
        picks, _, _ = asc.queue_model(geometry, asc.QUEUE_SEED, asc.QUEUE_SCHEDULE)
        q, pos = asc.initial_queue(geometry), cap
        for n in range(4 if batch == 1024 else 12):
            got, q = sq.parallel_dequeue(q, batch, sq.device_draws(asc.QUEUE_SEED, n, batch), pos, n_rec)
            pos += batch
            assert got == list(picks[n]), (geometry, n)


def test_wave_branch_runs_with_and_without_an_event():
    """from the draws alone: over the 20 batches run, a geometry of the wave branch with room for a batch without an event
    (capacity >= 4 batch) has batches of both kinds; the tight ones have an event in every batch"""
    nb = asc.schedule_batches(asc.QUEUE_SCHEDULE)
    roomy = 0
    for g in asc.QUEUE_GEOMETRIES:
        if g[1] > asc.WAVE:
            continue
        ev = asc.wave_events(g, asc.QUEUE_SEED, nb)
        print(g, "batches with an event: %d of %d" % (sum(ev), nb))
        if g[0] >= 4 * g[1]:
            roomy += 1
            assert any(ev) and not all(ev), g
        elif g[0] < 2 * g[1]:
            assert all(ev), g                                                   # a pick among the last `batch` slots is certain
    assert roomy >= 1
    assert any(asc.wave_events(asc.LARGE_GEOMETRY, asc.LARGE_SEED, 7, asc.LARGE_STATE[1]))


# ---- 2. air_batch_gather ----------------------------------------------------------------------------------------------
def test_gather_cases_reach_the_slice_boundary_and_every_mode():
    Cs = asc.GATHER_CASES
    assert len(Cs) == 18 and {(c["D"], c["batch"]) for c in Cs} == {(D, b) for D in asc.GATHER_D for b in asc.GATHER_BATCH}
    assert all(D % 4 == 0 for D in asc.GATHER_D) and 4 in asc.GATHER_D
    assert 4 * asc.GATHER_SLICE in asc.GATHER_D and 4 * asc.GATHER_SLICE + 4 in asc.GATHER_D
    assert {c["records"] for c in Cs} == set(asc.GATHER_RECORDS) and {c["mode"] for c in Cs} == set(asc.GATHER_MODES)
    for b in asc.GATHER_BATCH:
        assert {c["mode"] for c in Cs if c["batch"] == b} == set(asc.GATHER_MODES)
    for c in Cs:
        x = asc.gather_inputs(c)
        p = x["picks"]
        assert x["images"].shape == (c["records"], c["D"]) and p.shape == (c["batch"],) and p.min() >= 0 and p.max() < c["records"]
        assert c["records"] - 1 in p
        if c["batch"] >= 3:
            assert 0 in p and len(set(p.tolist())) < c["batch"]
        assert np.isfinite(x["images"]).all() and len(np.unique(x["images"])) > x["images"].size // 2


# ---- 3. air_summaries -------------------------------------------------------------------------------------------------
def test_summary_cases_cover_every_value():
    Cs = asc.SUMMARY_CASES
    assert {c["B"] for c in Cs} == set(asc.SUMMARY_B)
    assert {(c["N"], c["max_digits"], c["T"]) for c in Cs} == set(asc.SUMMARY_CONFIGS)
    for cfg in asc.SUMMARY_CONFIGS:
        Bs = [c["B"] for c in Cs if (c["N"], c["max_digits"], c["T"]) == cfg]
        assert min(Bs) < 64 and max(Bs) > 256, cfg
    assert {c["N"] for c in Cs} >= {1, 16} and {c["max_digits"] for c in Cs} >= {0, asc.SUMMARY_GROUPS_MAX}
    assert any(c["T"] < c["N"] for c in Cs) and any(c["T"] == c["N"] for c in Cs)


def test_summary_inputs_meet_their_conditions_and_the_reference_pads_with_zeros():
    read = [getattr(H, "ATT_" + n) for n in asc.SUMMARY_SLOTS]
    for c in asc.SUMMARY_CASES:
        B, N, md, T = c["B"], c["N"], c["max_digits"], c["T"]
        x = asc.summary_inputs(c)
        att = x["att"]
        other = [k for k in range(H.ATT_STRIDE) if k not in read + [H.ATT_MASK]]
        assert len(other) == 9 and np.isnan(att[..., other]).all()
        assert np.isfinite(att[:T][..., read]).all() and np.isnan(att[T:][..., read]).all()
        mask = att[..., H.ATT_MASK]
        assert (mask[:max(T - 1, 0)] > 0).any(axis=1).all() and not mask[max(T - 1, 0):].any()
        if T >= 2:
            assert (mask[0] > 0).sum() == 1                                     # a single image keeps the loop going
        assert x["digits"].min() >= 0 and x["digits"].max() <= N and x["targets"].min() >= 0 and x["targets"].max() <= md + 2
        ref = asc.summary_reference(c, x)
        names = osum.summary_names(N, md)
        assert ref.shape == (H.lib().air_summaries_count(N, md),) == (len(names),)
        d = dict(zip(names, ref))
        assert np.isnan(ref).any() and np.isfinite(ref[~np.isnan(ref)]).all() and d["loss"] == x["scalars"][0]
        if B >= 63:
            assert (x["targets"] > md).any()                                    # counted in _all_dig only
            assert (x["targets"] == x["lone"]).any() and np.isfinite(d["steps_%d_dig" % x["lone"]])
            assert np.isnan(d["scale_1_step_%d_dig" % x["lone"]]) and np.isfinite(d["z_pres_prob_1_step_%d_dig" % x["lone"]])
            if md >= 2:
                assert np.isnan(d["steps_%d_dig" % md]) and np.isfinite(d["steps_all_dig"])
            assert np.isfinite(d["rec_loss_all_dig"]) and d["rec_loss_all_dig"] != np.float32(
                x["rec_loss"][x["targets"] <= md].astype(np.float64).mean())
        # a column the loop did not reach is the zero padding, whatever the rows behind T' hold
        if T < N:
            assert d["z_pres_prob_%d_step_all_dig" % (T + 1)] == 0.0 and d["z_pres_prob_%d_step_all_dig" % T] > 0.0
            assert d["z_pres_kl_%d_step_all_dig" % N] == 0.0 or np.isnan(d["z_pres_kl_%d_step_all_dig" % N])
        assert asc.summary_ratio(ref, ref) == 0.0
        wrong = ref.copy()
        wrong[np.flatnonzero(~np.isnan(ref) & (ref != 0))[-1]] *= np.float32(1.000001)
        assert asc.summary_ratio(wrong, ref) > 1.0 and asc.summary_ratio(np.nan_to_num(ref), ref) == np.inf


# ---- 4. air_scene_records ---------------------------------------------------------------------------------------------
def test_scene_cases_and_stop_plans():
    assert len(asc.SCENE_CASES) == 10 and {c["given"] for c in asc.SCENE_CASES} == {0, 1}
    assert asc.scene_stops(4, 16) == slc.STOPS_B4 and asc.scene_stops(3, 5) == (None, 0, 2)
    assert asc.scene_stops(9, 16)[4:8] == slc.STOPS_B4                          # the plans repeat
    shapes = asc.SCENE_SHAPES
    assert any(B * N * ldz == B and B > pec.THREADS for B, N, Z, ldz, _ in shapes)       # the grid sized by B, two workgroups
    assert any(ldz > Z and z16 for _, _, Z, ldz, z16 in shapes) and any(ldz == Z and not z16 for _, _, Z, ldz, z16 in shapes)
    assert {N for _, N, _, _, _ in shapes} >= {1, 5, 16}


def test_scene_inputs_meet_their_margins_and_fp32_stays_within_a_quarter():
    worst = {}
    for c in asc.SCENE_CASES:
        B, N, Z, ldz = c["B"], c["N"], c["Z"], c["ldz"]
        x = asc.scene_inputs(c)
        ref = asc.scene_reference(c, x)
        m = asc.scene_margins(c, x, ref)
        assert m["S"] >= asc.S_MARGIN, (c, m)
        if c["given"]:
            assert m["relaxed"] >= 1e-6, (c, m)                                  # relaxed: no z_pres is 0 or 1
        else:
            assert m["round"] >= asc.ROUND_MARGIN, (c, m)
            for k in ("scale_src", "shift_src"):
                assert np.abs(x[k]).max() <= 2.5
            assert 0.0 < x["pres_src"].min() and x["pres_src"].max() < 1.0
        # the plan is met: the masks of the reference are the stop plan's
        mask_prev, mask = slc.expected_masks(x["stops"], N)
        assert np.array_equal(ref["att"][..., H.ATT_MASK], mask) and np.array_equal(ref["att"][..., H.ATT_MASK_PREV], mask_prev)
        assert np.isnan(x["dyn"]).sum() == H.DYN_COUNT - len(asc.SCENE_DYN)
        assert not ref["z"][..., Z:].any() and ref["z"].shape == (N, B, ldz)
        # the kernel's expressions in numpy fp32
        f32 = asc.scene_reference(c, x, np.float32)
        assert f32["att"].dtype == np.float32
        for name, k in asc.att_close_columns():
            worst[name] = max(worst.get(name, 0.0), asc.att_ratio(f32["att"][..., k], ref["att"][..., k]))
        for k in (H.ATT_Z, H.ATT_MASK_PREV, H.ATT_MASK):
            assert np.array_equal(f32["att"][..., k], ref["att"][..., k])
        if c["given"]:
            assert np.array_equal(f32["z"][..., :Z], x["z_src"])
        else:
            worst["z"] = max(worst.get("z", 0.0), pec.ratio(f32["z"][..., :Z], ref["z"][..., :Z], pec.REPARAM_FWD_TOL))
    print("fp32 restatement, largest error / bound:", {k: "%.4f" % v for k, v in sorted(worst.items())})
    assert all(v <= pec.QUARTER for v in worst.values()), worst
    assert set(worst) == {n for n, _ in asc.att_close_columns()} | {"z"}


def test_scene_reference_by_hand():
    """one image, two steps, given: the stopping sum in step order and theta_recon"""
    c = dict(B=1, N=2, Z=1, ldz=2, z16=False, given=1)
    x = dict(scale_src=np.array([[0.5], [0.25]], np.float32), shift_src=np.array([[[0.5, -0.25]], [[0.0, 0.5]]], np.float32),
             z_src=np.array([[[3.0]], [[4.0]]], np.float32), pres_src=np.array([[0.75], [0.125]], np.float32), dyn=slc.dyn_vector(1))
    a = asc.scene_reference(c, x)
    assert a["att"][0, 0].tolist() == [0.5, 0.5, -0.25, 0, 0.75, 0, 0, 0, 0, 0, 1, 1, 2, -1, 0.5, 0]       # S = 0.25 < 0.99
    assert a["att"][1, 0].tolist() == [0.25, 0, 0.5, 0, 0.125, 0, 0, 0, 0, 0, 1, 0, 4, 0, -2, 0]            # S = 1.125
    assert a["z"].tolist() == [[[3.0, 0.0]], [[4.0, 0.0]]]
    x = dict(x, pres_src=np.array([[0.5], [0.5]], np.float32))                  # u = 1/2: y = prior log-odds / T = -2.5 -> z = 0
    s = asc.scene_reference(dict(c, given=0), x)
    assert np.allclose(s["att"][:, 0, H.ATT_ZPRE], -2.5) and not s["att"][:, 0, H.ATT_Z].any()
    assert s["att"][:, 0, H.ATT_MASK_PREV].tolist() == [1, 0] and not s["att"][:, 0, H.ATT_MASK].any()
    assert np.allclose(s["z"][:, 0, 0], -0.125 + np.sqrt(0.75) * np.array([3.0, 4.0]))
    assert np.allclose(s["att"][0, 0, H.ATT_S], 1 / (1 + np.exp(1 - 0.5 * np.sqrt(np.float64(np.float32(0.05))))))


# ---- 5. air_render ----------------------------------------------------------------------------------------------------
def test_render_cases_reach_the_pixel_walk_edges_and_meet_the_tap_margin():
    T = asc.RENDER_THREADS
    assert asc.RENDER_FROM_WRITE == [(50, 28), (51, 28), (64, 32), (65, 32), (33, 7)] and asc.RENDER_ADDED == [(7, 2), (2, 2), (31, 5)]
    Cs = [C for C, _ in asc.RENDER_CASES]
    assert any(C * C < T for C in Cs) and any(C * C > T and T % C != 0 for C in Cs) and any(T % C == 0 and C * C > T for C in Cs)
    assert any(C * C < T and T % C != 0 for C, _ in asc.RENDER_ADDED) and (2, 2) in asc.RENDER_ADDED
    for C, w in asc.RENDER_ADDED:
        case, ref = asc.render_case_and_reference(C, w)
        assert ref["tap"] >= slc.WRITE_TAP_MARGIN, (C, w, ref["tap"])
        assert case["att"].shape == (16, 3, H.ATT_STRIDE) and case["vrec"].shape == (16, 3, w * w)
        assert case["vrec"].min() >= 0.02 and case["vrec"].max() <= 0.45       # the windows of slc._write_case_once
        assert ref["digits"].tolist() == [16, 7, 15] and ref["canvas"].shape == (3, C * C)
        assert ref["canvas"].min() >= 0.0 and ref["canvas"].max() <= 1.0 and ref["canvas"].std() > 0.01
        R = slc.running_recon64(case["att"], case["vrec"], C, w)
        assert np.array_equal(ref["canvas"], np.clip(R, 0.0, 1.0))
        a = asc.render_att(case["att"])
        assert np.isnan(a).sum() == 11 * 16 * 3 and np.array_equal(a[..., asc.RENDER_READS], case["att"][..., asc.RENDER_READS])
    case, ref = asc.render_case_and_reference(33, 7)                           # a shape of the compose cases IS that case
    wc, wr = slc.write_case_and_reference(33, 7, 50)
    assert case["att"] is wc["att"] and case["vrec"] is wc["vrec"] and ref["canvas"] is wr["recon"]
