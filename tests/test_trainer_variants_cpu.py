"""CPU: what the Trainer knows about every model variant without building one on a device -- the model table, the output adapter
table and the gradient all-reduce predicate per model."""
import torch

NAMES = ["Global_and_Local", "Global_and_Local_cyc_nofusion", "Foreground_and_Background", "Global_and_Local_Temporal",
         "Global_and_Local_conv_merge", "Global_only", "Global_only_cyc_nofusion", "Local_only", "model19", "Global_and_Local_CPS"]
BASELINES = ["baseline_unet", "multiview_unet", "early_fusion", "late_fusion", "MLP_fusion"]


def test_models_holds_the_fifteen_names():
    from glfusion_amd import engine, models as M
    assert sorted(engine.MODELS) == sorted(NAMES + BASELINES) and len(engine.MODELS) == 15
    for name in NAMES + BASELINES:
        assert engine.MODELS[name] is getattr(M, name)
    assert engine.NO_FUSION_FEATURES == tuple(BASELINES)


def test_adapter_table_has_a_row_per_model():
    from glfusion_amd import engine
    assert set(engine.OUTPUTS) == set(engine.MODELS)
    for name in NAMES:
        row = engine.OUTPUTS[name]
        assert row.heads == ((0, 1) if name == "Global_and_Local_CPS" else (0,)), name
        assert row.backbone == 1, name
        assert row.cycle == (3 if name == "Local_only" else 2), name
        assert row.clip_is_video == (name == "Global_and_Local_Temporal"), name
    for name in BASELINES:
        assert engine.OUTPUTS[name] == engine.Outputs(heads=(0,), backbone=None, cycle=None, clip_is_video=False), name


def test_reducer_predicate_keeps_the_shared_encoders_of_the_cps_model():
    from glfusion_amd import engine, ddp
    from glfusion_amd.models import Global_and_Local_CPS
    model = Global_and_Local_CPS(["1"])
    ignore = engine.reducer_ignore("Global_and_Local_CPS")
    names = [n for n, _ in model.named_parameters()]
    kept = {n for n in names if not ignore(n)}
    # network 2's encoders ARE the template's: listed under network.backbone.*, reached by the loss, reduced
    assert "network.backbone.conv1.weight" in names and "network.backbone.conv1.weight" in kept
    assert "network.backbone.layer4.2.bn3.weight" in kept
    assert model.layer4_2["1"][2].bn3.weight is model.network.backbone["layer4"][2].bn3.weight
    # the template's head stays dead; so does align_channel
    assert "network.classifier.4.weight" in names and "network.classifier.4.weight" not in kept
    assert not any(n.startswith("network.") and not n.startswith("network.backbone.") for n in kept)
    assert not any("align_channel" in n for n in kept)
    assert all(ignore(n) == ddp.default_ignore(n) for n in names if not n.startswith("network."))
    # the reducer built with it lists them (world size 1: no collective, no device)
    red = ddp.GradAllReducer(model, ignore=ignore)
    assert "network.backbone.conv1.weight" in red.names and "network.classifier.4.weight" not in red.names
    assert "network.backbone.conv1.weight" not in ddp.GradAllReducer(model).names


def test_every_other_model_keeps_the_default_predicate():
    from glfusion_amd import engine, ddp
    for name in NAMES + BASELINES:
        if name != "Global_and_Local_CPS":
            assert engine.reducer_ignore(name) is ddp.default_ignore, name
