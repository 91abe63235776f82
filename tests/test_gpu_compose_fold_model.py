"""AIRModel(compose_fold=...): the captured train steps run compose inside the write-backward launch
(air_write_fwd_bwd) where the library has that form -- one launch fewer, the same training bit for bit; the eager step,
train_step_ops() and the models without that form keep their lists."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import air_oracle as ao  # noqa: E402
from oracle.synth import blob_canvases  # noqa: E402

HP = dict(ao.TRAINING_HP)
KERNEL = "compose_write_bwd_graph_kernel"


@pytest.fixture(scope="module")
def am():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from air import air_model
    return air_model


def _model(am, images, targets, hp=HP, **kw):
    am.reset_default_graph()
    return am.AIRModel(torch.tensor(images, device="cuda"), torch.tensor(targets, device="cuda"), cnn=False, train=True,
                       annealing_schedules=ao.TRAINING_ANNEALING, seed=0, noise_seed=0, gemm_precision="bf16", **kw, **hp)


def _state(model):
    torch.cuda.synchronize()
    st = model.store
    return dict(params=st.params.clone(), m=st.m.clone(), v=st.v.clone(), grads=st.grads.clone(), loss=model.loss.clone(),
                accuracy=model.accuracy.clone(), reconstruction=model.reconstruction.clone(),
                loss_per_item=model.loss_per_item.clone(), digits=model.rec_num_digits.clone(), step=int(st.istate[0]))


def _same(a, b):
    for k in a:
        if k == "step":
            assert a[k] == b[k]
        else:
            assert torch.equal(a[k], b[k]), k


def test_two_replays_of_two_steps_equal_four_eager_steps_and_the_two_launch_graph(am):
    B = 8
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=3)
    params = ao.init_params(HP, 0)

    eager = _model(am, images, targets)
    eager.load_state_dict(params)
    for _ in range(4):
        eager.training(eager=True)
    e4 = _state(eager)
    assert eager.captured_step_ops() is None
    assert len(eager.train_step_ops()) == 23

    states = {}
    for fold in (True, False):
        model = _model(am, images, targets, compose_fold=fold)
        model.load_state_dict(params)
        model.capture_graph(steps=2)
        eager_ops = model.train_step_ops()
        assert len(eager_ops) == 23
        for step in (0, 1):
            ops = model.captured_step_ops(step)
            names = [op.name for op in ops]
            if fold:
                assert len(ops) == len(eager_ops) - 1 == 22
                assert names.count("compose_write_bwd") == 1 and "compose_fwd" not in names and "write_bwd" not in names
                fused = ops[names.index("compose_write_bwd")]
                assert fused is model._fold_op and fused.kernel == KERNEL
                # everything else is the eager step's op, in its order (the x.Wx launch apart: the twin-operand form at step 1)
                rest = [op for op in eager_ops if op.name not in ("compose_fwd", "write_bwd")]
                assert [op.name for op in ops if op is not fused][1:] == [op.name for op in rest][1:]
                assert names.index("compose_write_bwd") == [op.name for op in eager_ops].index("compose_fwd")
            else:
                assert model._fold_op is None
                assert names[1:] == [op.name for op in eager_ops][1:]
                assert [op.kernel for op in ops][1:] == [op.kernel for op in eager_ops][1:]
        model.training()
        model.training()
        states[fold] = _state(model)
        assert states[fold]["step"] == 4
        assert int(model._arrive.item()) == 0
    _same(e4, states[True])
    _same(e4, states[False])


def test_models_without_the_form_capture_their_two_launches(am):
    """the exact adjoint has no graph-order launch to fold into; at 128 x 128 one tap's terms are resident at a time"""
    B = 4
    images, targets = blob_canvases(B, HP["canvas_size"], HP["max_digits"], seed=5)
    exact = _model(am, images, targets, backward="exact")
    exact.capture_graph()
    assert exact._fold_op is None
    assert [op.kernel for op in exact.captured_step_ops()] == [op.kernel for op in exact.train_step_ops()]
    exact.release_graph()

    hp = dict(HP, canvas_size=128)
    images, targets = blob_canvases(B, 128, hp["max_digits"], seed=5)
    big = _model(am, images, targets, hp=hp)
    big.capture_graph()
    assert big._fold_op is None
    kernels = [op.kernel for op in big.captured_step_ops()]
    assert kernels == [op.kernel for op in big.train_step_ops()]
    assert "write_fwd_kernel<1024>" in kernels and "write_bwd_graph_kernel<false>" in kernels
    torch.cuda.synchronize()
