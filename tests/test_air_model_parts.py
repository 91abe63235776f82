"""air_model.py in parts: what moved to air/_store.py, air/_generate.py and air/summaries.py is still reached through
air_model under the names callers use -- as the very objects of the new modules, not as copies."""
import types


def test_air_model_re_exports_the_objects_of_its_parts():
    from air import _generate, _store, air_model as am
    for name in ("VariableStore", "_SCOPES", "xavier_uniform_", "reset_default_graph", "saved_cnn_arguments"):
        assert getattr(am, name) is getattr(_store, name), name
    assert am.GeneratedScenes is _generate.GeneratedScenes
    assert am._st_matrices is _generate.st_matrices and am.st_matrices is _generate.st_matrices
    assert am.GEMM_PRECISION in ("fp32", "bf16")
    # one registry: a scope dropped through air_model is dropped in the store's module
    _store._SCOPES["parts"] = None
    am.reset_default_graph()
    assert _store._SCOPES == {} and am._SCOPES is _store._SCOPES


def test_summary_names_are_loss_accuracy_and_the_numeric_names():
    from air import air_model as am
    from air.summaries import numeric_names
    names = am.AIRModel.summary_names(types.SimpleNamespace(max_steps=3, max_digits=2))
    assert names == ["loss", "accuracy"] + numeric_names(3, 2)
    assert len(names) == 90 and len(set(names)) == 90
