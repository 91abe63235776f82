"""GPU test of the driver loop that carries the evaluation instruments (training.py: SummaryWriter with instruments=): all
three air.metrics instruments through push() / flush() on a real inference model, in process, against the instruments'
own values() taken by hand on the same passes.  (What each instrument computes: the GPU tests of each.)"""
import json
import time

import numpy as np
import pytest
import torch

import abi_check as abi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def H():
    return abi.gpu_hip()


def _rounded(values):
    return [round(v, 5) if v == v else None for v in values]


def test_all_three_instruments_through_the_summary_writer(H, tmp_path):
    """AIRModel(cnn=False, train=False) at B = 8, T = 3 on scenes a DeviceSceneSource composed from a small handwriting bank,
    which is also the ground truth.  Two evaluations, at steps 0 and 50, with the z_pres bias raised in between so that
    the passes differ (a row that came out of the wrong slot of a ring would show)."""
    import multi_mnist as mm
    import training
    from air import air_model as am
    from air.metrics import LatentProbe, Localization, Segmentation
    from oracle import air_oracle as ao
    hp = dict(ao.TRAINING_HP)
    B, G, Cc = 8, 2, hp["canvas_size"]
    am.reset_default_graph()
    images = torch.zeros(B, Cc ** 2, device="cuda")
    digits = torch.zeros(B, dtype=torch.int32, device="cuda")
    model = am.AIRModel(images, digits, cnn=False, train=False, scope="instruments8", gemm_precision="fp32", **hp)
    params = {k: np.array(v) for k, v in ao.init_params(hp, 0).items()}
    bias = "z_pres/log_odds/output/biases"
    bank, base_labels = mm.handwriting_bank(64, 11, torch.device("cuda", 0))
    bank.refresh()
    source = mm.DeviceSceneSource(bank, B, images, digits, canvas_dim=Cc, max_digits=G, seed=5)
    source.next_batch()
    for raised in range(12):
        model.load_state_dict(params)
        model.forward()
        if int(model.run_digits.sum()) >= 4:
            break
        params[bias] = params[bias] + np.float32(1.0)
    meta = source.meta()
    of_variant = torch.from_numpy(bank.labels(base_labels).astype(np.int32)).cuda()
    labels = of_variant[meta["indices"].long().clamp(min=0)].view(B, G).contiguous()
    boxes = (digits, meta["positions"], meta["boxes"])
    instruments = [(Localization(model, G), boxes), (Segmentation(model, G), (Segmentation.scene_masks(source, digits),)),
                   (LatentProbe(model, G, k=3, max_distance=2.9), boxes + (labels,))]
    calls = []
    writer = training.SummaryWriter(model, str(tmp_path / "scalars.jsonl"), time.perf_counter(),
                                    on_row=lambda step, values: calls.append((step, "row", values)), instruments=instruments,
                                    on_values=lambda step, instrument, values: calls.append((step, type(instrument).__name__, values)))
    want = {}
    for step in (0, 50):
        model.forward()
        writer.push(step)
        by_hand = []
        for instrument, truth in instruments:                       # the same pass, scored from zero once more
            instrument.evaluate(*truth)
            by_hand.append(instrument.values().cpu().tolist())
        want[step] = (model.numeric_summaries().cpu().tolist(), by_hand)
        params[bias] = params[bias] + np.float32(1.0)
        model.load_state_dict(params)
    writer.flush()
    writer.file.close()
    rows = [json.loads(line) for line in open(tmp_path / "scalars.jsonl")]
    assert [r["step"] for r in rows] == [0, 50]
    names = model.summary_names()
    keys = [i.prefix + k for i, _ in instruments for k in i.reported]
    assert len(keys) == 13 and keys[0] == "loc_mean_iou" and keys[5] == "seg_fg_ari" and keys[9] == "lat_knn_accuracy"
    print("z_pres bias raised %d times" % raised)
    for r in rows:
        summaries, by_hand = want[r["step"]]
        assert list(r) == ["step", "wall_s"] + names + keys
        assert [r[k] for k in names] == _rounded(summaries)                  # as without instruments
        for (instrument, _), values in zip(instruments, by_hand):
            got = dict(zip(instrument.names(), _rounded(values)))
            print(r["step"], type(instrument).__name__, got)
            assert {k: r[instrument.prefix + k] for k in instrument.reported} == {k: got[k] for k in instrument.reported}
        assert "loc_count_accuracy" not in r
    assert rows[0] != dict(rows[1], step=0, wall_s=rows[0]["wall_s"])        # the two passes differ
    assert rows[0]["loc_mean_iou"] is not None and rows[0]["seg_mask_iou"] is not None and rows[0]["lat_scored"] is not None
    # the callbacks: on_row, then the instruments in list order, with the values of their reported names
    assert [(c[0], c[1]) for c in calls] == [(s, n) for s in (0, 50) for n in ("row", "Localization", "Segmentation", "LatentProbe")]
    for step, name, values in calls:
        summaries, by_hand = want[step]
        if name == "row":
            assert np.array_equal(np.asarray(values), np.asarray(summaries), equal_nan=True)
            continue
        (instrument, _), full = next((i, v) for i, v in zip(instruments, by_hand) if type(i[0]).__name__ == name)
        reported = [dict(zip(instrument.names(), full))[k] for k in instrument.reported]
        assert np.asarray(values).tobytes() == np.asarray(reported).tobytes(), (step, name)
