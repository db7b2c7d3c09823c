"""Fused global-norm gradient clipping with non-finite step skipping (glf_grad_sumsq, glf_grad_clip_coef, the clipped forms of
glf_adam_step / glf_sgd_step, glf_grad_scale; optim.*.set_grad_clip, optim.grad_norm, optim.clip_grad_norm_) against the host and
against torch.optim on CPU copies whose gradients were multiplied by the coefficient the device reported.

The tolerances of the update tests are those of tests/test_gpu_optim.py (rtol 2e-6; atol 1e-8 parameters, 1e-7 exp_avg, 1e-9
exp_avg_sq) and tests/test_gpu_sgd.py (rtol 2e-6; atol 1e-8 parameters, 1e-7 momentum buffer), which fix the scale of the data:
parameters 0.3 * randn, |gradient| < 0.25, lr <= 0.01.  Here the raw gradients are 1e3 * randn, but what enters the update is
g * coef with coef ~ 1 / (1e3 * sqrt(65 955)): about 4e-3 * randn, inside that scale.  The clipped kernel adds one exactly
specified float multiply, which the CPU side repeats (g * coef in float32), so nothing new enters the error."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 1 << 16
# [1]; [7]: scalar tail only; [3, 5]: its GRADIENT is a view 4 bytes off a 16-byte boundary (scalar path throughout);
# [8, 4, 3, 3]: vector path only; [CHUNK + 3]: two table rows, the second ragged (3 elements); [5]: never receives a gradient
SHAPES = [(1,), (7,), (3, 5), (8, 4, 3, 3), (CHUNK + 3,), (5,)]
MISALIGNED, RAGGED, NO_GRAD = 2, 4, 5
LR = 0.01
SGD_CONFIGS = [(0, 0, False, 0), (0, 0, False, 1e-4), (0.9, 0, False, 1e-4), (0.9, 0.1, False, 0), (0.9, 0, True, 1e-4)]


def _values(seed, scale):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * scale for s in SHAPES]


def _pair(seed):
    """The same parameters twice, CPU and device, each as two param groups with different learning rates."""
    vals = _values(seed, 0.3)
    cpu = [torch.nn.Parameter(v.clone()) for v in vals]
    gpu = [torch.nn.Parameter(v.clone().to(DEV)) for v in vals]
    return cpu, gpu


def _groups(params, lr=LR):
    return [{"params": params[:3], "lr": lr}, {"params": params[3:], "lr": 0.5 * lr}]


def _grads(seed):
    """Seeded randn * 1e3 (the parameter at NO_GRAD gets none): clipping is active at max_norm = 1."""
    gs = _values(seed, 1e3)
    gs[NO_GRAD] = None
    return gs


def _to_device(g, i):
    if g is None:
        return None
    if i == MISALIGNED:
        big = torch.zeros(64, device=DEV)
        view = big[1:16].view(3, 5)
        view.copy_(g)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        return view
    return g.clone().to(DEV)


def _set(gpu, grads, skip=()):
    for i, (p, g) in enumerate(zip(gpu, grads)):
        p.grad = None if i in skip else _to_device(g, i)


def _set_cpu(cpu, grads, coef, skip=()):
    """The CPU twin's gradients: g * coef, one float32 multiply, as the clipped kernel forms it."""
    c = torch.tensor(coef, dtype=torch.float32)
    for i, (p, g) in enumerate(zip(cpu, grads)):
        p.grad = None if g is None or i in skip else g * c


def _host_norm(grads, skip=()):
    total = sum(float((g.double() ** 2).sum()) for i, g in enumerate(grads) if g is not None and i not in skip)
    return np.float32(math.sqrt(total))


def _bits(t):
    return int(t.detach().cpu().view(torch.int32))


def _assert_norm(got, grads, what, skip=()):
    """Equal to the float32 rounding of the host's double result or its float32 neighbour: the kernel accumulates in double
    (own error about n * 2^-53), so the one rounding that shows is the conversion to float."""
    want = _host_norm(grads, skip)
    got = np.float32(float(got))
    print(f"{what}: device {got!r} host {want!r}")
    assert got in (want, np.nextafter(want, np.float32(np.inf)), np.nextafter(want, np.float32(-np.inf))), what


def _host_coef(max_norm, norm):
    with np.errstate(over="ignore"):
        return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(norm) + np.float32(1e-6)))


def _close(got, want, what, rtol=2e-6, atol=1e-8):
    got, want = got.detach().cpu().numpy(), want.detach().numpy()
    err = np.abs(got - want)
    print(f"{what}: max abs err {err.max():.3e}, max err / (atol + rtol |ref|) {(err / (atol + rtol * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


def _snapshot(opt, gpu):
    return [p.detach().clone() for p in gpu], {(i, k): v.clone() for i, p in enumerate(gpu) for k, v in opt.state.get(p, {}).items()
                                               if isinstance(v, torch.Tensor) and v.is_cuda}


# ---------------------------------------------------------------------------------------------------------------- 1. the norm
def test_norm_of_a_step_and_of_the_free_function():
    from glfusion_amd import optim
    cpu, gpu = _pair(0)
    grads = _grads(10)
    _set(gpu, grads)
    opt = optim.SGD(_groups(gpu), lr=LR)
    opt.set_grad_clip(1.0)
    opt.step()
    assert opt.grad_norm.dtype == torch.float32 and opt.grad_norm.is_cuda and opt.grad_norm.dim() == 0
    assert opt.skipped_steps.dtype == torch.int64 and opt.skipped_steps.is_cuda and int(opt.skipped_steps) == 0
    _assert_norm(opt.grad_norm, grads, "optimizer.grad_norm")
    free = optim.grad_norm(gpu)
    assert free.dtype == torch.float32 and free.is_cuda and free.dim() == 0
    _assert_norm(free, grads, "optim.grad_norm")
    # the same bits from run to run and from both routes (one table against a combined one changes no row)
    assert _bits(free) == _bits(optim.grad_norm(gpu)) == _bits(opt.grad_norm)
    # the parameter without a gradient does not contribute, whatever it holds; one that loses its gradient drops out
    with torch.no_grad():
        gpu[NO_GRAD].fill_(1e30)
    assert _bits(optim.grad_norm(gpu)) == _bits(free)
    gpu[3].grad = None
    _assert_norm(optim.grad_norm(gpu), grads, "optim.grad_norm without parameter 3", skip=(3,))
    _assert_norm(optim.grad_norm(gpu[0]), [grads[0]], "optim.grad_norm of one tensor")


# --------------------------------------------------------------------------------------------------------- 2. the coefficient
@pytest.mark.parametrize("max_norm", [1.0, 1e12, math.inf])
def test_coefficient_is_torchs_expression_on_the_reported_norm(max_norm):
    from glfusion_amd import optim
    cpu, gpu = _pair(0)
    _set(gpu, _grads(11))
    opt = optim.Adam(gpu, lr=3e-4)                                           # one group, one class: the norm runs over the update's own table
    opt.set_grad_clip(max_norm)
    opt.step()
    norm, coef = np.float32(float(opt.grad_norm)), np.float32(float(opt.clip_coef))
    want = _host_coef(max_norm, norm)
    print(f"max_norm {max_norm}: norm {norm!r} coef {coef!r} expected {want!r}")
    assert coef.tobytes() == want.tobytes()
    assert (coef < 1e-5) if max_norm == 1.0 else (coef == 1.0)
    assert int(opt.skipped_steps) == 0


# ----------------------------------------------------------------------------------------------------------- 3. the update
@pytest.mark.parametrize("wd,late", [(0.0, False), (1e-5, False), (1e-5, True)])
def test_clipped_adam_matches_torch_adam_on_scaled_gradients(wd, late):
    """late: parameter 1 gets its first gradient at step 2 -- two classes (step counts), one norm over both."""
    from glfusion_amd.optim import Adam
    cpu, gpu = _pair(1)
    ref, opt = torch.optim.Adam(_groups(cpu, 3e-4), weight_decay=wd), Adam(_groups(gpu, 3e-4), weight_decay=wd)
    opt.set_grad_clip(1.0)
    launches = []
    real = opt._launch
    opt._launch = lambda group, t, table: (launches.append(t), real(group, t, table))
    for step in range(3):
        grads = _grads(100 + step)
        skip = (1,) if late and step < 2 else ()
        _set(gpu, grads, skip)
        kept = [None if p.grad is None else p.grad.clone() for p in gpu]
        del launches[:]
        opt.step()
        if late and step == 2:
            assert sorted(launches) == [1, 3, 3]                          # first group: the late parameter's class and the others'
        for p, k in zip(gpu, kept):                                          # p.grad is left unscaled, bit for bit
            assert (p.grad is None and k is None) or torch.equal(p.grad, k)
        _assert_norm(opt.grad_norm, grads, f"norm step {step}", skip=skip)
        coef = float(opt.clip_coef)
        assert 0 < coef < 1e-5
        _set_cpu(cpu, grads, coef, skip)
        ref.step()
        for i, (a, b) in enumerate(zip(cpu, gpu)):
            _close(b, a, f"param {i} step {step}")
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        if i == NO_GRAD:
            assert b not in opt.state
            continue
        sa, sb = ref.state[a], opt.state[b]
        assert int(sa["step"]) == int(sb["step"])
        _close(sb["exp_avg"], sa["exp_avg"], f"exp_avg {i}", atol=1e-7)
        _close(sb["exp_avg_sq"], sa["exp_avg_sq"], f"exp_avg_sq {i}", atol=1e-9)
    assert int(opt.skipped_steps) == 0


@pytest.mark.parametrize("momentum,dampening,nesterov,wd", SGD_CONFIGS)
def test_clipped_sgd_matches_torch_sgd_on_scaled_gradients(momentum, dampening, nesterov, wd):
    from glfusion_amd.optim import SGD
    cpu, gpu = _pair(2)
    kw = dict(lr=LR, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd)
    ref, opt = torch.optim.SGD(_groups(cpu), **kw), SGD(_groups(gpu), **kw)
    opt.set_grad_clip(1.0)
    untouched = gpu[NO_GRAD].detach().clone()
    for step in range(3):
        grads = _grads(200 + step)
        _set(gpu, grads)
        kept = [None if p.grad is None else p.grad.clone() for p in gpu]
        opt.step()
        for p, k in zip(gpu, kept):
            assert (p.grad is None and k is None) or torch.equal(p.grad, k)
        _assert_norm(opt.grad_norm, grads, f"norm step {step}")
        _set_cpu(cpu, grads, float(opt.clip_coef))
        ref.step()
        for i, (a, b) in enumerate(zip(cpu, gpu)):
            _close(b, a, f"param {i} step {step}")
    assert gpu[NO_GRAD] not in opt.state and torch.equal(gpu[NO_GRAD].detach(), untouched)
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        if momentum == 0 or i == NO_GRAD:
            assert b not in opt.state or len(opt.state[b]) == 0
            continue
        assert set(opt.state[b]) == {"momentum_buffer"} == set(ref.state[a])
        _close(opt.state[b]["momentum_buffer"], ref.state[a]["momentum_buffer"], f"momentum buffer {i}", atol=1e-7)
    assert copy.deepcopy(opt.state_dict())["param_groups"] == ref.state_dict()["param_groups"]


# ------------------------------------------------------------------------------------------------------ 4. the default path
def _run_plain(make, clip):
    cpu, gpu = _pair(3)
    opt = make(gpu)
    if clip == "on-then-off":
        opt.set_grad_clip(1.0)
        opt.set_grad_clip(None)
    elif clip is not None:
        opt.set_grad_clip(clip)
    for step in range(3):
        _set(gpu, _values(300 + step, 0.03)[:NO_GRAD] + [None], skip=(1,) if step == 0 else ())
        opt.step()
    return _snapshot(opt, gpu)


@pytest.mark.parametrize("which", ["adam", "sgd", "sgd-momentum"])
def test_default_path_is_bit_identical(which):
    """Never set, set and unset, and float('inf') on finite gradients (coef = 1, g * 1 is exact): the same bits."""
    from glfusion_amd.optim import SGD, Adam
    make = {"adam": lambda p: Adam(_groups(p, 3e-4), weight_decay=1e-5), "sgd": lambda p: SGD(_groups(p), lr=LR, weight_decay=1e-4),
            "sgd-momentum": lambda p: SGD(_groups(p), lr=LR, momentum=0.9, dampening=0.1, weight_decay=1e-4)}[which]
    params0, state0 = _run_plain(make, None)
    for clip in ("on-then-off", math.inf):
        params, state = _run_plain(make, clip)
        assert all(torch.equal(a, b) for a, b in zip(params0, params)), clip
        assert state.keys() == state0.keys() and all(torch.equal(state0[k], state[k]) for k in state0), clip


# ------------------------------------------------------------------------------------------------- 5. non-finite gradients
def _poison(grads, bad):
    grads = [None if g is None else g.clone() for g in grads]
    grads[RAGGED][CHUNK + 1] = bad                                           # in the ragged second row
    return grads


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_adam_skips_a_non_finite_step(bad):
    from glfusion_amd.optim import Adam
    cpu, gpu = _pair(4)
    ref, opt = torch.optim.Adam(_groups(cpu, 3e-4), weight_decay=1e-5), Adam(_groups(gpu, 3e-4), weight_decay=1e-5)
    opt.set_grad_clip(1.0)
    grads = _grads(400)
    _set(gpu, grads)
    opt.step()
    _set_cpu(cpu, grads, float(opt.clip_coef))
    ref.step()
    params, state = _snapshot(opt, gpu)
    assert len(state) == 2 * (len(SHAPES) - 1)
    _set(gpu, _poison(_grads(401), bad))
    opt.step()
    assert int(opt.skipped_steps) == 1 and float(opt.clip_coef) == 0.0
    norm = float(opt.grad_norm)
    assert math.isinf(norm) if math.isinf(bad) else math.isnan(norm)
    params1, state1 = _snapshot(opt, gpu)
    assert all(torch.equal(a, b) for a, b in zip(params, params1))
    assert state.keys() == state1.keys() and all(torch.equal(state[k], state1[k]) for k in state)
    # the host-side step count has advanced all the same (documented): mirror it in the twin, then one finite step on both
    for st in ref.state.values():
        st["step"] += 1
    grads = _grads(402)
    _set(gpu, grads)
    opt.step()
    assert int(opt.skipped_steps) == 1
    _set_cpu(cpu, grads, float(opt.clip_coef))
    ref.step()
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        _close(b, a, f"param {i} after the skipped step")
        if i != NO_GRAD:
            assert int(ref.state[a]["step"]) == int(opt.state[b]["step"]) == 3
            _close(opt.state[b]["exp_avg"], ref.state[a]["exp_avg"], f"exp_avg {i}", atol=1e-7)
            _close(opt.state[b]["exp_avg_sq"], ref.state[a]["exp_avg_sq"], f"exp_avg_sq {i}", atol=1e-9)


@pytest.mark.parametrize("bad", [math.inf, math.nan])
@pytest.mark.parametrize("skip_at", [0, 1])
@pytest.mark.parametrize("momentum,dampening,nesterov,wd", [(0.9, 0.1, False, 1e-4), (0.9, 0, True, 0)])
def test_sgd_skips_a_non_finite_step(bad, skip_at, momentum, dampening, nesterov, wd):
    """skip_at = 0: the skipped step is the one that would have written the first momentum buffers; the next finite step must
    then BE the first step (buf = d, not momentum * buf + (1 - dampening) * d), as it is for torch, which never saw the
    skipped one."""
    from glfusion_amd.optim import SGD
    cpu, gpu = _pair(5)
    kw = dict(lr=LR, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd)
    ref, opt = torch.optim.SGD(_groups(cpu), **kw), SGD(_groups(gpu), **kw)
    opt.set_grad_clip(1.0)
    for step in range(3):
        if step == skip_at:
            params, state = _snapshot(opt, gpu)
            _set(gpu, _poison(_grads(500 + step), bad))
            opt.step()
            assert int(opt.skipped_steps) == 1 and float(opt.clip_coef) == 0.0
            params1, state1 = _snapshot(opt, gpu)
            assert all(torch.equal(a, b) for a, b in zip(params, params1))
            assert all(torch.equal(state[k], state1[k]) for k in state)          # every buffer that existed: not a bit moved
            if skip_at == 1:
                assert state.keys() == state1.keys()
            continue
        grads = _grads(500 + step)
        _set(gpu, grads)
        opt.step()
        _set_cpu(cpu, grads, float(opt.clip_coef))
        ref.step()
        for i, (a, b) in enumerate(zip(cpu, gpu)):
            _close(b, a, f"param {i} step {step}")
            if i != NO_GRAD:
                _close(opt.state[b]["momentum_buffer"], ref.state[a]["momentum_buffer"], f"momentum buffer {i} step {step}", atol=1e-7)
    assert int(opt.skipped_steps) == 1


def test_sgd_leaving_clipped_mode_after_a_skipped_first_step():
    """The buffers of a skipped first step hold no values; with clipping switched off they leave the state again, and the next
    (unclipped) step is torch's first step."""
    from glfusion_amd.optim import SGD
    cpu, gpu = _pair(6)
    kw = dict(lr=LR, momentum=0.9, dampening=0.1, weight_decay=1e-4)
    ref, opt = torch.optim.SGD(_groups(cpu), **kw), SGD(_groups(gpu), **kw)
    opt.set_grad_clip(1.0)
    _set(gpu, _poison(_grads(600), math.nan))
    opt.step()
    opt.set_grad_clip(None)
    assert all("momentum_buffer" not in opt.state.get(p, {}) for p in gpu)
    grads = _values(601, 0.03)[:NO_GRAD] + [None]
    _set(gpu, grads)
    _set_cpu(cpu, grads, 1.0)
    opt.step()
    ref.step()
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        _close(b, a, f"param {i}")
        if i != NO_GRAD:
            _close(opt.state[b]["momentum_buffer"], ref.state[a]["momentum_buffer"], f"momentum buffer {i}", atol=1e-7)


@pytest.mark.parametrize("bad", [math.inf, math.nan])
def test_clip_grad_norm_leaves_non_finite_gradients_alone(bad):
    from glfusion_amd import optim
    cpu, gpu = _pair(7)
    _set(gpu, _poison(_grads(700), bad))
    kept = [None if p.grad is None else p.grad.clone() for p in gpu]
    norm = float(optim.clip_grad_norm_(gpu, 1.0))
    assert math.isinf(norm) if math.isinf(bad) else math.isnan(norm)
    for p, k in zip(gpu, kept):
        assert (p.grad is None and k is None) or torch.equal(p.grad.view(torch.int32), k.view(torch.int32))


# ---------------------------------------------------------------------------------------------- 6. clip_grad_norm_ in place
def test_clip_grad_norm_in_place_then_an_unclipped_step():
    from glfusion_amd import optim
    cpu, gpu = _pair(8)
    grads = _grads(800)
    _set(gpu, grads)
    ptrs = [None if p.grad is None else p.grad.data_ptr() for p in gpu]
    norm = optim.clip_grad_norm_(gpu, 1.0)
    assert norm.dtype == torch.float32 and norm.is_cuda and norm.dim() == 0
    _assert_norm(norm, grads, "clip_grad_norm_")
    coef = torch.tensor(_host_coef(1.0, np.float32(float(norm))))
    assert 0 < float(coef) < 1e-5
    for i, (p, g) in enumerate(zip(gpu, grads)):
        if g is None:
            assert p.grad is None
            continue
        assert p.grad.data_ptr() == ptrs[i]                                  # in place
        assert torch.equal(p.grad.cpu(), g * coef), i                        # one float multiply: bit-exact
    # not clipping: nothing changes
    kept = [None if p.grad is None else p.grad.clone() for p in gpu]
    optim.clip_grad_norm_(gpu, 1e12)
    optim.clip_grad_norm_(gpu, math.inf)
    assert all(k is None or torch.equal(p.grad, k) for p, k in zip(gpu, kept))
    # a following unclipped step against torch's own spelling on the CPU copies
    for a, g in zip(cpu, grads):
        a.grad = None if g is None else g.clone()
    t_norm = torch.nn.utils.clip_grad_norm_(cpu, 1.0)
    # torch's norm is a float32 sum: off by at most log2(65 539) * 2^-24 ~ 1e-6 relative, which moves the step by 1e-6 * 4e-5
    print(f"torch's norm {float(t_norm)!r} ours {float(norm)!r}")
    assert abs(float(t_norm) - float(norm)) <= 1e-5 * float(norm)
    kw = dict(lr=LR, momentum=0.9, weight_decay=1e-4)
    ref, opt = torch.optim.SGD(_groups(cpu), **kw), optim.SGD(_groups(gpu), **kw)
    ref.step()
    opt.step()
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        _close(b, a, f"param {i}")
        if i != NO_GRAD:
            _close(opt.state[b]["momentum_buffer"], ref.state[a]["momentum_buffer"], f"momentum buffer {i}", atol=1e-7)


# --------------------------------------------------------------------------------------------------------------- 7. Trainer
TRAINER_LR = 0.1


def _cfg(save_dir, graph):
    opt = {"opt_name": "SGD", "lr": TRAINER_LR, "params": (0.9, 0.999), "weight_decay": 0.0}
    tr = {"batch_size": 1, "frames_per_clip": 2, "num_epochs": 1, "clip_length": 8, "view_num": ["1", "3"], "test_view": ["1", "3"],
          "dense_cyc": False, "save_dir": str(save_dir), "iters_per_epoch": 2, "global_rank": 0, "validate_every_epoch": False,
          "clip_grad_norm": 1.0, "graph": graph}
    return {"train": tr, "net": {"opt": opt}}


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_clips_every_sgd_step(tmp_path, graph, capsys):
    """A clipped plain-SGD step with weight_decay 0 moves the parameters by lr * coef * |g| <= lr * max_norm in global L2 norm;
    the bound asserted is lr * (1 + 1e-5).  What the float32 update p + (-lr * coef * g) adds to that is its rounding: at most half
    an ulp of p per element, so at most 2^-24 * |all parameters| in global norm (printed below), which enters the norm of the
    step in quadrature.  The learning rate is chosen so that this stays far below the 1e-5: a step of 0.1 spread over tens of
    millions of elements is ~1e-5 per element, three orders above an ulp of a weight of 0.05; at lr = 1e-4 the per-element step
    (~1e-8) would be of the size of that ulp and the measured norm mostly rounding."""
    from glfusion_amd.engine import Trainer
    from glfusion_amd.optim import SGD
    t = Trainer(_cfg(tmp_path, graph))
    assert type(t.optimizer) is SGD and t.optimizer._max_norm == 1.0
    params = [p for p in t.model.parameters()]
    pnorm = math.sqrt(float(sum((p.detach().double() ** 2).sum() for p in params)))
    print(f"|parameters| {pnorm:.4g}: rounding of one update <= {2.0 ** -24 * pnorm:.3g} in global norm")
    moves, norms = [], []
    real = t.train_step

    def measured(*args, **kw):
        before = [p.detach().clone() for p in params]
        out = real(*args, **kw)
        sq = sum(((p.detach().double() - b.double()) ** 2).sum() for p, b in zip(params, before))
        moves.append(math.sqrt(float(sq)))
        norms.append(float(t.optimizer.grad_norm))
        return out
    t.train_step = measured
    t.train(is_backbone=False, is_cycle=False)
    print(f"graph {graph}: moves {moves} gradient norms {norms}")
    assert len(moves) == 2
    for move, norm in zip(moves, norms):
        assert math.isfinite(norm) and norm > 0
        assert move <= TRAINER_LR * (1 + 1e-5)
        if norm > 1.0:
            assert move >= TRAINER_LR * (1 - 1e-4)                            # clipping, not shrinking: the step has norm lr
    assert int(t.optimizer.skipped_steps) == 0
    out = capsys.readouterr().out
    print(out)
    assert "grad-norm" in out and "skipped-steps 0" in out
