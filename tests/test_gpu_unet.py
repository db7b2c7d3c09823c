"""GPU: baseline_unet / multiview_unet (glfusion_amd.models; GLfusion/models/ours.py:2416-2625) against fixtures made by the
reference's own classes (tests/golden/unet_*.npz), a train step against the plain-torch restatement tests/unet_ref.py in float64,
and the Trainer's model switch."""
import copy
import os
import shutil

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import glfusion_ref as orc   # the checker (tests only)

import unet_ref

DEV = "cuda"
VIEWS, INPUTS = unet_ref.VIEWS, unet_ref.INPUTS
NAMES = ("baseline_unet", "multiview_unet")


def close(a, b, tol):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    err = (a - b).abs()
    ok = bool((err <= tol + tol * b.abs()).all())
    if not ok:
        print("max abs err", float(err.max()), "max |ref|", float(b.abs().max()))
    return ok


def _sample(t, k):
    flat = t.reshape(-1)
    idx = np.unique(np.linspace(0, flat.numel() - 1, num=min(k, flat.numel())).astype(np.int64))
    return flat[torch.from_numpy(idx).to(flat.device)]


@pytest.mark.parametrize("tag", sorted(INPUTS))
@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16", "bf16"])
@pytest.mark.parametrize("name", NAMES)
def test_unet_eval_vs_golden(golden_dir, name, prec, tag):
    """Eval outputs against the reference's own classes.  f32 / f16x3: logit samples to 1e-4, x5 to 1e-3 (the gate of
    test_variants_eval_vs_golden).  f16: within 2e-2 of the largest logit (the mode's own tolerance, test_f16_mode_parity).
    bf16 (16-bit storage): relative to the largest logit, 3x the deviation of the restatement with a bf16 round-trip at every stored
    tensor (summation order and the once-rounded BatchNorm differ from the emulation), never looser than the 6e-2 of
    test_s16_e2e_eval_vs_golden.  The emulation's deviation (unet_ref.BF16_DEVIATION, measured on the CPU and re-measured by
    tests/test_unet_ref_cpu.py): baseline_unet 1.53e-2 (112 x 112) / 1.67e-2 (48 x 32) -> limits 4.59e-2 / 5.01e-2; multiview_unet
    3.78e-2 / 1.63e-2 -> limits 6e-2 (the cap; 3x would be 1.13e-1) / 4.89e-2."""
    import glfusion_amd.models as M
    from glfusion_amd import ops
    g = np.load(os.path.join(golden_dir, f"unet_{name}.npz"))
    n, h, w = INPUTS[tag]
    model = getattr(M, name)(VIEWS)
    assert list(model.state_dict().keys()) == [str(k) for k in g["keys"]]
    orc.closed_form_fill(model, salt=9)
    model = model.to(DEV).eval()
    imgs = {v: t.to(DEV) for v, t in orc.closed_form_images(VIEWS, n, h, w).items()}
    with ops.precision_scope(prec):
        with torch.no_grad():
            out = model(imgs)
        torch.cuda.synchronize()
    assert out[1] is None and out[2] is None
    for v in VIEWS:
        assert tuple(out[0][v].shape) == (n, 5, h, w) and out[0][v].dtype == torch.float32 and out[0][v].is_contiguous()
        assert tuple(out[3][v].shape) == (n, 1024, h // 16, w // 16)
        got, want = _sample(out[0][v], 20011).cpu(), torch.from_numpy(g[f"mask_{tag}:{v}"])
        got5, want5 = _sample(out[3][v].float(), 4099).cpu(), torch.from_numpy(g[f"x5_{tag}:{v}"])
        rel = float((got - want).abs().max()) / float(want.abs().max())
        print(f"{name} {prec} {tag} view {v}: logit error {rel:.3e} of the largest logit; x5 {float((got5 - want5).abs().max()):.3e}")
        if prec in ("f32", "f16x3"):
            assert close(got, want, 1e-4), v
            assert close(got5, want5, 1e-3), v
        elif prec == "f16":
            assert rel <= 2e-2, (v, rel)
        else:
            dev = unet_ref.BF16_DEVIATION[name][tag]
            limit = min(3.0 * dev, 6e-2)
            print(f"  bf16 emulation deviation {dev:.3e} -> limit {limit:.3e}")
            assert rel <= limit, (v, rel, dev, limit)
            assert bool(torch.isfinite(got5).all())


def test_unet_refuses_sizes_that_are_no_multiple_of_16():
    import glfusion_amd.models as M
    m = M.multiview_unet(["1"]).to(DEV).eval()
    with pytest.raises(RuntimeError, match="multiples of 16"):
        m({"1": torch.zeros(1, 1, 48, 40, device=DEV)})


# ------------------------------------------------------------------------------------------------------------------ train step
def _restatement_grads_64_and_32(ref, loss_of):
    """Gradients of the restatement's float64 evaluation, and the relative L2 deviation of its OWN float32 evaluation from them per
    tensor (what any fp32 arithmetic is entitled to on that tensor)."""
    r32 = copy.deepcopy(ref).float().train()
    loss_of(r32, torch.float32).backward()
    r64 = ref.double().train()
    want = loss_of(r64, torch.float64)
    want.backward()
    g64 = {k: p.grad for k, p in r64.named_parameters() if p.grad is not None}
    noise = {k: float((p.grad.double() - g64[k]).norm()) / max(float(g64[k].norm()), 1e-30) for k, p in r32.named_parameters() if k in g64}
    return float(want.detach()), g64, noise, r64


def _gate_all_gradients(model, gref, noise32, label, base=2e-3, operand_bits=22):
    """The rule of tests/test_gpu_model.py::_gate_all_gradients: every parameter gradient against the float64 evaluation to relative
    L2 <= 2e-3, or 10x the restatement's own fp32-vs-fp64 deviation on that tensor x 2^(24 - operand_bits) where that is larger
    (split-fp16 x3 operands carry 22 bits), + a floor of 2e-5 of the largest gradient norm in the parameter's top-level module (a
    bias in front of a train-mode BatchNorm has a structurally zero gradient: only the floor gates it)."""
    scale = {}
    for k, w in gref.items():
        scale[k.split(".")[0]] = max(scale.get(k.split(".")[0], 0.0), float(w.norm()))
    worst = (0.0, "", 0.0)
    for k, p in model.named_parameters():
        if k not in gref:
            continue
        want = gref[k].double()
        err = float((p.grad.double().cpu() - want).norm())
        rel_tol = max(base, 10.0 * 2.0 ** (24 - operand_bits) * noise32.get(k, 0.0))
        tol = rel_tol * float(want.norm()) + 2e-5 * scale[k.split(".")[0]]
        if err / tol > worst[0]:
            worst = (err / tol, k, err / max(float(want.norm()), 1e-30))
        assert err <= tol, (label, k, err, float(want.norm()), tol, noise32.get(k))
    print(f"{label}: closest to its gate: {worst[1]} at {worst[0]:.2f} of the tolerance (relative L2 {worst[2]:.2e})")


@pytest.mark.parametrize("name", ["multiview_unet", "baseline_unet"])
def test_unet_train_step_vs_restatement(name):
    """Train step on the kink-free fill (no ReLU input near zero), 3 frames of 48 x 32, BCE-sum over head 0, precision f16x3: the
    loss to 2e-6, EVERY parameter gradient by the rule above, the same set of parameters with a gradient (180 of 180 for
    baseline_unet; 192 of 194 for multiview_unet, global_attn.align_channel.* is dead), BatchNorm running statistics to 1e-4."""
    import glfusion_amd.models as M
    from glfusion_amd import ops
    n, h, w = 3, 48, 32
    ref = getattr(unet_ref, name)(VIEWS)
    orc.kinkfree_fill(ref, salt=9)
    sd0 = {k: v.clone() for k, v in ref.state_dict().items()}
    imgs = orc.varied_images(VIEWS, n, h, w)
    tgts = orc.closed_form_targets(VIEWS, n, c=5, h=h, w=w)

    def loss_of(net, dt):
        o = net({v: t.to(dt) for v, t in imgs.items()})
        return sum(torch.nn.functional.binary_cross_entropy_with_logits(o[0][v], tgts[v].to(dt), reduction="sum") for v in VIEWS)
    want, gref, noise32, ref = _restatement_grads_64_and_32(ref, loss_of)
    assert len(gref) == {"baseline_unet": 180, "multiview_unet": 192}[name]
    print(f"{name}: restatement fp32-vs-fp64 gradient deviation, largest {max(noise32.values()):.2e}")
    model = getattr(M, name)(VIEWS)
    model.load_state_dict(sd0, strict=True)
    model = model.to(DEV).train()
    with ops.precision_scope("f16x3"):                           # the bench's arithmetic
        out = model({v: t.to(DEV) for v, t in imgs.items()})
        got = sum(ops.bce_with_logits_sum(out[0][v], tgts[v].to(DEV)) for v in VIEWS)
        got.backward()
        torch.cuda.synchronize()
    print(f"{name}: loss {float(got.detach()):.6f}, float64 {want:.6f}")
    assert abs(float(got.detach()) - want) <= 2e-6 * abs(want)
    have = {k for k, p in model.named_parameters() if p.grad is not None}
    assert have == set(gref), have ^ set(gref)
    _gate_all_gradients(model, gref, noise32, name)
    sd, sd_ref = model.state_dict(), ref.state_dict()
    for k in sd:
        if "running_" in k or k.endswith("num_batches_tracked"):
            assert close(sd[k].float(), sd_ref[k].float(), 1e-4), k


# --------------------------------------------------------------------------------------------------------------------- Trainer
def _cfg(save_dir, model="multiview_unet", opt_name="Adam", num_epochs=2, **train):
    tr = {"batch_size": 1, "frames_per_clip": 2, "num_epochs": num_epochs, "clip_length": 8, "view_num": list(VIEWS), "test_view": list(VIEWS),
          "dense_cyc": False, "save_dir": str(save_dir), "iters_per_epoch": 1, "global_rank": 0, "validate_every_epoch": False}
    tr.update(train)
    net = {"opt": {"opt_name": opt_name, "lr": 1e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}
    if model is not None:
        net["model"] = model
    return {"train": tr, "net": net}


def _run_epochs(cfg):
    from glfusion_amd.engine import Trainer
    torch.manual_seed(0)
    t = Trainer(cfg)
    losses = []
    real = t.train_step

    def recorded(*args, **kw):
        out = real(*args, **kw)
        losses.append(float(out[0]))
        return out
    t.train_step = recorded
    t.train(is_backbone=False, is_cycle=False)
    t.train_step = real
    return t, losses


def test_trainer_runs_multiview_unet_eagerly_from_a_graph_and_resumes(tmp_path):
    """Two epochs of one iteration with config['net']['model'] = 'multiview_unet', eagerly and with graph: True: finite losses that
    agree to the 1e-4 the graph-replayed Global_and_Local step is held to (test_trainer_graph_mode_follows_the_eager_trainer: the
    recorded step runs the same kernels on other streams).  A Trainer resumed from the eager run's checkpoint reproduces the loss of
    the eager Trainer's next step on the same batch; eval() returns the Dice of the synthetic patients."""
    from glfusion_amd import models as M
    from glfusion_amd.engine import Trainer
    d_e, d_g = os.path.join(str(tmp_path), "eager"), os.path.join(str(tmp_path), "graph")
    try:
        eager, le = _run_epochs(_cfg(d_e, save_optimizer=True))
        assert type(eager.model) is M.multiview_unet and eager.model_name == "multiview_unet"
        graph, lg = _run_epochs(_cfg(d_g, graph=True))
        assert graph._graph is not None
        print("eager", le, "graph", lg)
        assert len(le) == 2 and len(lg) == 2 and all(np.isfinite(x) for x in le + lg) and le[0] != le[1]
        for a, b in zip(le, lg):
            assert abs(a - b) <= 1e-4 * abs(a), (le, lg)
        del graph
        # resume: the third step, on one batch, from the live Trainer and from its checkpoint
        resumed = Trainer(_cfg(d_e, num_epochs=3, is_load=True, save_optimizer=True))
        assert resumed.latest_epoch == 2 and type(resumed.model) is M.multiview_unet
        batch = eager.loader.batch()
        eager.model.train(); resumed.model.train()
        la, lb = float(eager.train_step(*batch)[0]), float(resumed.train_step(*batch)[0])
        print("next step: live", la, "resumed", lb)
        assert np.isfinite(la) and abs(la - lb) <= 1e-5 * abs(la), (la, lb)
        out = resumed.eval()
        assert set(out) == set(VIEWS) and all(np.isfinite(x) and 0.0 <= x <= 1.0 for v in VIEWS for x in out[v])
        with pytest.raises(ValueError, match="multiview_unet"):
            resumed.train(is_backbone=False, is_cycle=True)
        with pytest.raises(ValueError, match="multiview_unet"):
            resumed.cycle_loss(batch[0])
    finally:
        shutil.rmtree(str(tmp_path), ignore_errors=True)


def test_trainer_runs_baseline_unet_with_sgd_and_clipping(tmp_path):
    from glfusion_amd import models as M
    cfg = _cfg(tmp_path, model="baseline_unet", opt_name="SGD", num_epochs=1, clip_grad_norm=1.0)
    cfg["net"]["opt"]["momentum"] = 0.9
    try:
        t, losses = _run_epochs(cfg)
        assert type(t.model) is M.baseline_unet and len(losses) == 1 and np.isfinite(losses[0])
        assert np.isfinite(float(t.optimizer.grad_norm)) and int(t.optimizer.skipped_steps) == 0
        assert set(t.reducer.names) == {k for k, _ in t.model.named_parameters()}          # every parameter of this model gets a gradient
        sd = torch.load(os.path.join(str(tmp_path), "net_00000.pth"), map_location="cpu")["network"]
        unet_ref.baseline_unet(VIEWS).load_state_dict(sd, strict=True)                     # the reference's key set accepts the checkpoint
    finally:
        shutil.rmtree(str(tmp_path), ignore_errors=True)


def test_trainer_validation_and_visual_passes_run_baseline_unet(tmp_path):
    """validation_and_test and test_visualize take the one mask these models return (there is no backbone mask to choose)."""
    from glfusion_amd import data
    from glfusion_amd.engine import Trainer
    t = Trainer(_cfg(tmp_path, model="baseline_unet", num_epochs=1, eval_patients=1))
    infos = data.synthetic_infos(VIEWS, 4, 8, device="cpu", seed=91)
    dice = t.validation_and_test(net_root=None, is_fuse=False, raw_data=False, infos=infos, reduce=False)
    assert np.isfinite(dice) and 0.0 <= dice <= 1.0
    assert set(t.validation_report["Inner-test"]) == set(VIEWS)
    man = t.test_visualize("unet", out_root=os.path.join(str(tmp_path), "vis"), nifti=False, overlay_alpha=None)
    assert set(man) == {"0_0"} and set(man["0_0"]) == set(VIEWS)
    for v in VIEWS:
        assert man["0_0"][v]["frames"] == 8 and os.path.exists(os.path.join(man["0_0"][v]["png_dir"], "pred_7.png"))
    shutil.rmtree(str(tmp_path), ignore_errors=True)


def test_trainer_model_switch_default_and_unknown_name(tmp_path):
    from glfusion_amd import models as M
    from glfusion_amd.engine import Trainer
    with pytest.raises(ValueError, match="config\\['net'\\]\\['model'\\]"):
        Trainer(_cfg(tmp_path, model="unet_plus_plus"))
    t = Trainer(_cfg(tmp_path, model=None, view_num=["1"], test_view=["1"]))
    assert type(t.model) is M.Global_and_Local and t.model_name == "Global_and_Local"
