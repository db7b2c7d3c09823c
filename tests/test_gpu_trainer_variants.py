"""GPU: the Trainer builds, trains, checkpoints, scores and renders every variant of the main network (engine.MODELS / engine.OUTPUTS),
and the cross pseudo supervision step of Global_and_Local_CPS is the step composed by hand from the pieces it fuses."""
import os

import numpy as np
import pytest
import torch

from oracle import glfusion_ref as orc   # the checker (tests only)

pytestmark = pytest.mark.gpu
DEV = "cuda"

NAMES = ["Global_and_Local", "Global_and_Local_cyc_nofusion", "Foreground_and_Background", "Global_and_Local_Temporal",
         "Global_and_Local_conv_merge", "Global_only", "Global_only_cyc_nofusion", "Local_only", "model19", "Global_and_Local_CPS"]


def _cfg(tmp_path, name, views=("1",), **train):
    """the config of test_trainer_surface_runs_cycle_training_and_checkpoints (tests/test_gpu_engine.py) for model `name`"""
    cfg = {"train": {"batch_size": 2, "num_epochs": 1, "clip_length": 29, "view_num": list(views), "test_view": list(views), "dense_cyc": True,
                     "save_dir": str(tmp_path), "iters_per_epoch": 1, "global_rank": 0, "validate_every_epoch": False},
           "net": {"model": name, "opt": {"opt_name": "Adam", "lr": 3e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}}
    cfg["train"].update(train)
    return cfg


def _classifier_weight(model, name):
    return (model.classifier_1 if name == "Global_and_Local_CPS" else model.classifier)["1"][4].weight


@pytest.mark.parametrize("name", NAMES)
def test_trainer_trains_checkpoints_scores_and_renders_every_variant(tmp_path, name):
    from glfusion_amd.data import SyntheticPatients
    from glfusion_amd.engine import Trainer
    t = Trainer(_cfg(tmp_path, name))
    calls = []
    if name == "Global_and_Local_Temporal":              # forward spy: which calls are told they carry one video
        inner = t.model.forward

        def spy(x, is_video=False):
            calls.append((int(x["1"].shape[0]), bool(is_video)))
            return inner(x, is_video=is_video)
        t.model.forward = spy
    before = _classifier_weight(t.model, name).detach().clone()
    t.train(is_backbone=False, is_cycle=True)
    assert not torch.equal(before, _classifier_weight(t.model, name))
    if name == "Global_and_Local_Temporal":
        assert calls == [(2, False), (29, True)], calls      # the labelled batch, then the clip
        del t.model.forward
    ckpt = os.path.join(str(tmp_path), "net_00000.pth")
    assert os.path.exists(ckpt)
    sd = torch.load(ckpt, map_location="cpu")["network"]
    getattr(orc, name)(["1"]).load_state_dict(sd, strict=True)          # the oracle's class of the same name accepts it
    patients = SyntheticPatients(["1"], 1, clip_length=3, h0=150, w0=170, device=DEV, seed=5)
    for is_fuse in (True, False):
        out = t.eval(net_path=ckpt, is_fuse=is_fuse, patients=patients)
        assert set(out) == {"1"} and all(np.isfinite(x) for x in out["1"]), (is_fuse, out)
    man = t.test_visualize(name, out_root=os.path.join(str(tmp_path), "vis"), patients=patients, nifti=False, overlay_alpha=None)
    assert set(man) == {"0_0"} and man["0_0"]["1"]["frames"] == 3
    assert sorted(os.listdir(man["0_0"]["1"]["png_dir"])) == sorted(f"{kind}_{i}.png" for kind in ("pred", "gnd") for i in range(3))
    if name == "Local_only":
        # the cycle term acts on out[3], the local-fusion features: taken from out[2], the detached gate map, this gradient would be None
        t.model.train()
        for p in t.model.parameters():
            p.grad = None
        t.cycle_loss(t.video_loader.batch()[0]).backward()
        g = t.model.local_attn.W_z[1].weight.grad                  # the block's BatchNorm scale: reached whatever its (zero) initial value
        assert g is not None and float(g.abs().max()) > 0.0


def test_cps_weight_needs_the_cps_model(tmp_path):
    from glfusion_amd.engine import Trainer
    with pytest.raises(ValueError, match="cps_weight"):
        Trainer(_cfg(tmp_path, "Global_and_Local", cps_weight=0.5))
    with pytest.raises(ValueError, match="cps_weight"):
        Trainer(_cfg(tmp_path, "baseline_unet", cps_weight=0.5))


def test_cps_term_on_patient_batches_needs_patient_clips(tmp_path):
    """config['train']['infos'] without ['video_infos']: the refusal of train(is_cycle=True) also holds for the CPS term's clip"""
    from glfusion_amd import data
    from glfusion_amd.engine import SyntheticClips, Trainer
    from test_gpu_data_batch import _infos
    infos = _infos()
    t = Trainer(_cfg(tmp_path, "Global_and_Local_CPS", views=("4",), cps_weight=0.5, clip_length=24, infos=infos, train_list=list(infos)))
    assert isinstance(t.loader, data.BatchLoader) and isinstance(t.video_loader, SyntheticClips)
    with pytest.raises(ValueError, match="video_infos"):
        t.train(is_backbone=False, is_cycle=False)
    assert t.clip_cycle is True


def test_cps_step_is_the_step_composed_by_hand(tmp_path):
    """Trainer.train_step with cps_weight = 0.5 (A) against the same step written out with model(imgs), model(video),
    ops.bce_with_logits_sum on both heads and on the thresholded, detached masks of the other network, and ops.dense_seg_cycle (B),
    from the same weights: two runs of one step under one precision, compared at the gates of
    tests/test_gpu_engine.py::test_step_graph_replay_matches_eager_step.  A pseudo label that differs between the runs at a pixel
    whose logit is within rounding of 0 moves the loss by that |logit| and a gradient by one pixel's share of ~1e5."""
    from glfusion_amd import ops
    from glfusion_amd.engine import Trainer
    views, w = ["1", "3"], 0.5

    def make():
        t = Trainer(_cfg(tmp_path, "Global_and_Local_CPS", views, cps_weight=w))
        orc.kinkfree_fill(t.model, salt=7)
        orc.set_dropout(t.model, 0.0)
        t.model.train()
        return t
    A, B = make(), make()
    B.model.load_state_dict(A.model.state_dict(), strict=True)
    imgs, masks = A.loader.batch()
    video = A.video_loader.batch()[0]
    names = [n for n, _ in A.model.named_parameters()]
    assert "network.backbone.conv1.weight" in A.reducer.names          # network 2's shared encoder takes part in the all-reduce
    assert "network.classifier.4.weight" not in A.reducer.names

    loss_a, pred = A.train_step(imgs, masks, video)
    assert pred is not None and set(pred) == set(views)
    ga = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in A.model.named_parameters()}

    out = B.model(imgs)
    clip = B.model(video)
    total = None
    for head in (0, 1):
        for v in views:
            l = ops.bce_with_logits_sum(out[head][v], masks[v])
            total = l if total is None else total + l
    cross = None
    for v in views:
        m1u, m2u = clip[0][v], clip[1][v]
        l = ops.bce_with_logits_sum(m1u, (m2u.detach() > 0).float()) + ops.bce_with_logits_sum(m2u, (m1u.detach() > 0).float())
        cross = l if cross is None else cross + l
    feats = ops.pooled_fusion_features(clip[2])
    cyc = None
    for v in views:
        l = ops.dense_seg_cycle(feats[v], 16, 2, 3, 10, soft_label=False, is_overlap=True)
        cyc = l if cyc is None else cyc + l
    total = total + w * cross + 1e-2 * cyc
    for p in B.model.parameters():
        p.grad = None
    total.backward()
    torch.cuda.synchronize()
    la, lb = float(loss_a), float(total.detach())
    print(f"CPS step: trainer loss {la!r}, by hand {lb!r}, rel {abs(la - lb) / abs(lb):.3g}; cps term {float(cross.detach())!r}")
    assert float(cross.detach()) > 0.0
    gb = {n: p.grad for n, p in B.model.named_parameters()}
    floor = 2e-5 * max(float(g.norm()) for g in gb.values() if g is not None)
    worst = (0.0, None)
    for n in names:
        if gb[n] is None:
            assert ga[n] is None, n
            continue
        assert ga[n] is not None, n
        err, ref = float((ga[n] - gb[n]).norm()), float(gb[n].norm())
        rel = 1e-2 if ".convs.4." in n else 1e-3
        worst = max(worst, (err / (rel * ref + floor), n))
    print(f"CPS step: largest gradient error / gate {worst[0]:.3g} at {worst[1]}")
    assert abs(la - lb) <= 1e-6 * abs(lb), (la, lb)
    for n in names:
        if gb[n] is not None:
            err, ref = float((ga[n] - gb[n]).norm()), float(gb[n].norm())
            rel = 1e-2 if ".convs.4." in n else 1e-3
            assert err <= rel * ref + floor, (n, err, ref, floor)
    assert float(ga["network.backbone.conv1.weight"].abs().max()) > 0.0
    assert ga["network.classifier.4.weight"] is None


def test_cps_training_reports_the_agreement_and_draws_a_clip_without_the_cycle_term(tmp_path, capsys):
    from glfusion_amd.engine import Trainer
    views = ["1", "3"]
    t = Trainer(_cfg(tmp_path, "Global_and_Local_CPS", views, cps_weight=0.5))
    assert t.cps_report == {}
    drawn = []
    batch = t.video_loader.batch
    t.video_loader.batch = lambda: (drawn.append(1), batch())[1]
    t.train(is_backbone=False, is_cycle=False)                 # no cycle term: the clip is drawn for the CPS term alone
    assert len(drawn) == 1
    assert set(t.cps_report) == set(views) and all(0.0 <= x <= 1.0 for x in t.cps_report.values()), t.cps_report
    assert "cps-agreement" in capsys.readouterr().out


def test_cps_model_graph_step_follows_its_eager_step(tmp_path):
    """config['train']['graph'] with cps_weight = 0: the recorded core supervises both heads.  The gates of
    tests/test_gpu_engine.py::test_trainer_graph_mode_follows_the_eager_trainer."""
    from glfusion_amd import ops
    from glfusion_amd.engine import Trainer
    ops.set_precision("f16x3")
    try:
        def make(graph):
            cfg = _cfg(tmp_path, "Global_and_Local_CPS", batch_size=4, iters_per_epoch=3, clip_length=8, graph=graph)
            cfg["net"]["opt"] = {"opt_name": "Adam", "lr": 1e-5, "weight_decay": 1e-5}
            torch.manual_seed(0)
            t = Trainer(cfg)
            orc.kinkfree_fill(t.model, salt=9)
            orc.set_dropout(t.model, 0.0)
            t.model.train()
            return t
        eager, graph = make(False), make(True)
        keys = ("layer4_1.1.2.conv3.weight", "network.backbone.layer4.2.conv3.weight", "classifier_2.1.4.weight")
        start = {k: eager.model.state_dict()[k].clone() for k in keys}
        batches = [eager.loader.batch() for _ in range(3)]
        le = [float(eager.train_step(i, m)[0]) for i, m in batches]
        lg = [float(graph.train_step(i, m)[0]) for i, m in batches]
        assert graph._graph is not None
        for a, b in zip(le, lg):
            assert abs(a - b) <= 1e-4 * abs(a), (le, lg)
        assert len({round(x, 1) for x in lg}) == 3
        pe, pg = ({n: p.detach() for n, p in t.model.named_parameters()} for t in (eager, graph))
        for k in keys:                                          # network 1, network 2's shared encoder, network 2's head: all move, together
            assert float((pe[k] - pg[k]).norm()) <= 5e-3 * float(pe[k].norm()), k
            assert float((pg[k] - start[k]).norm()) > 0.0, k
        graph._graph.release()
    finally:
        ops.set_precision("f32")
