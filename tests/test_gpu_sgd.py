"""Fused multi-tensor SGD (glf_sgd_step, glfusion_amd.optim.SGD) against torch.optim.SGD on CPU copies -- the 'SGD' branch of
the reference's optimizer switch (GLfusion/main.py:158-161) plus momentum / dampening / nesterov as torch defines them."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
# [1]; [7]: scalar tail only; [3, 5]: storage 4 bytes off a 16-byte boundary (scalar path throughout); [65 537]: crosses the
# 65 536-element chunk row, 1-element tail row; [64, 64, 3, 3]: vector path only; [5]: never receives a gradient
SHAPES = [(1,), (7,), (3, 5), (65537,), (64, 64, 3, 3), (5,)]
NO_GRAD = 5
CONFIGS = [(0, 0, False, 0), (0, 0, False, 1e-4), (0.9, 0, False, 1e-4), (0.9, 0.1, False, 0), (0.9, 0, True, 1e-4)]
# The tolerances are test_adam_matches_torch_adam's: rtol 2e-6 everywhere, atol 1e-8 on parameters and 1e-7 on the moving
# average.  The absolute parts are what the two roundings of a * b + c (this kernel, by design) may differ by from the single one
# of ATen's CPU kernels (vec::fmadd) where the terms cancel: at most half an ulp of the product plus the ulp by which an input of
# the step already differs.  They fix the scale of the data:
#   momentum buffer: gradients of 0.03 * randn stay below 0.25 (8 sigma), where an ulp is <= 1.5e-8, so one step adds at most
#     0.75e-8 + 1.5e-8 and the recursion err' = 0.9 err + that, over the five updates of a buffer, at most 4.1 times it: 9.2e-8.
#     (At 0.3 * randn the same bound is 8 times larger, and a numpy model of the kernel's arithmetic does exceed 1e-7.)
#   parameter: one step adds at most lr_t * (error of the direction, <= 1.5e-7) + half an ulp of lr_t * direction (<= 2.3e-10 for
#     lr_t * 0.6 < 2^-7); the cosine schedule's lr_t sum to 3.0 LR, so LR = 0.01 bounds it by 4.5e-9 + 1.4e-9 < 1e-8.
# A wrong term in the update (a dropped dampening, weight decay or momentum factor) moves a buffer by >= 1e-4 and a parameter by
# >= 1e-6 at these scales, orders above the tolerances.
LR = 0.01
PARAM_SCALE, GRAD_SCALE = 0.3, 0.03


def _values(seed, scale=PARAM_SCALE):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) * scale for s in SHAPES]


def _pair(seed):
    """The same parameters twice: CPU (for torch.optim.SGD) and device (for ours).  The [3, 5] one is a contiguous view at an
    odd element offset of a larger buffer, so its data pointer is not 16-byte aligned."""
    cpu, gpu = [], []
    for s, v in zip(SHAPES, _values(seed)):
        cpu.append(torch.nn.Parameter(v.clone()))
        if s == (3, 5):
            big = torch.zeros(64, device=DEV)
            view = big[1:16].view(3, 5)
            view.copy_(v)
            assert view.is_contiguous() and view.data_ptr() % 16 == 4
            gpu.append(torch.nn.Parameter(view))
        else:
            gpu.append(torch.nn.Parameter(v.clone().to(DEV)))
    return cpu, gpu


def _set_grads(cpu, gpu, seed, skip=()):
    for i, (a, b, g) in enumerate(zip(cpu, gpu, _values(seed, GRAD_SCALE))):
        if i == NO_GRAD or i in skip:
            a.grad = b.grad = None
        else:
            a.grad = g.clone()
            b.grad = g.clone().to(DEV)


def _close(got, want, what, rtol=2e-6, atol=1e-8):
    got, want = got.detach().cpu().numpy(), want.detach().numpy()
    err = np.abs(got - want)
    print(f"{what}: max abs err {err.max():.3e}, max err / (atol + rtol |ref|) {(err / (atol + rtol * np.abs(want))).max():.3f}")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize("momentum,dampening,nesterov,wd", CONFIGS)
def test_sgd_matches_torch_sgd(momentum, dampening, nesterov, wd):
    from glfusion_amd.optim import SGD
    cpu, gpu = _pair(0)
    kw = dict(lr=LR, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd)
    ref, opt = torch.optim.SGD(cpu, **kw), SGD(gpu, **kw)
    sched_r = torch.optim.lr_scheduler.CosineAnnealingLR(ref, T_max=5)        # main.py:168
    sched_o = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=5)
    untouched = gpu[NO_GRAD].detach().clone()
    for step in range(6):
        _set_grads(cpu, gpu, 100 + step)
        ref.step()
        opt.step()
        sched_r.step()
        sched_o.step()
        assert opt.param_groups[0]["lr"] == ref.param_groups[0]["lr"]
        for i, (a, b) in enumerate(zip(cpu, gpu)):
            _close(b, a, f"param {i} step {step}")
    # the parameter without a gradient: no state, not a bit moved
    assert gpu[NO_GRAD] not in opt.state and torch.equal(gpu[NO_GRAD].detach(), untouched)
    for i, (a, b) in enumerate(zip(cpu, gpu)):
        if momentum == 0 or i == NO_GRAD:
            assert b not in opt.state or len(opt.state[b]) == 0
            continue
        assert set(opt.state[b]) == {"momentum_buffer"} == set(ref.state[a])
        # absolute tolerance at operand scale: see the note on LR / GRAD_SCALE above
        _close(opt.state[b]["momentum_buffer"], ref.state[a]["momentum_buffer"], f"momentum buffer {i}", atol=1e-7)
    assert copy.deepcopy(opt.state_dict())["param_groups"] == ref.state_dict()["param_groups"]


@pytest.mark.parametrize("momentum,dampening,nesterov,wd", [c for c in CONFIGS if c[0] != 0])
def test_sgd_state_dict_round_trip_through_torch(momentum, dampening, nesterov, wd):
    """Three steps here, the state into torch.optim.SGD and back, one more step on both sides.  Parameter 1 gets its first
    gradient only after the reload: the "first buffer" and the "has a buffer" launches occur in that one step."""
    from glfusion_amd.optim import SGD
    late = 1
    cpu, gpu = _pair(1)
    kw = dict(lr=LR, momentum=momentum, dampening=dampening, nesterov=nesterov, weight_decay=wd)
    opt = SGD(gpu, **kw)
    for step in range(3):
        _set_grads(cpu, gpu, 200 + step, skip=(late,))
        opt.step()
    assert gpu[late] not in opt.state and gpu[NO_GRAD] not in opt.state
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"]) == {0, 2, 3, 4} and all(set(s) == {"momentum_buffer"} for s in sd["state"].values())
    twin = [torch.nn.Parameter(b.detach().cpu().clone()) for b in gpu]
    t_opt = torch.optim.SGD(twin, **kw)
    t_opt.load_state_dict(sd)                        # torch's own SGD accepts the state ...
    back = SGD(gpu, **kw)
    back.load_state_dict(t_opt.state_dict())         # ... and ours accepts torch's
    _set_grads(twin, gpu, 300)
    launches = []
    real = back._launch
    back._launch = lambda group, first, table: (launches.append(first), real(group, first, table))
    back.step()
    t_opt.step()
    assert sorted(launches) == [False, True]
    for i, (b, t) in enumerate(zip(gpu, twin)):
        _close(b, t, f"param {i} after the reload")
        if i != NO_GRAD:
            _close(back.state[b]["momentum_buffer"], t_opt.state[t]["momentum_buffer"], f"momentum buffer {i} after the reload", atol=1e-7)


def test_sgd_step_bumps_the_version_of_exactly_the_updated_parameters():
    from glfusion_amd.optim import SGD
    cpu, gpu = _pair(2)
    opt = SGD(gpu, lr=LR, momentum=0.9)
    for step, skip in enumerate([(), (0, 3), ()]):
        _set_grads(cpu, gpu, 400 + step, skip=skip)
        before = [p._version for p in gpu]
        opt.step()
        for i, p in enumerate(gpu):
            assert p._version == before[i] + (0 if i == NO_GRAD or i in skip else 1), (step, i)


def test_conv_forward_after_sgd_step_uses_the_new_weights():
    """The kernel writes the parameters through raw pointers; every weight-derived image of the split-fp16 convolution (tap-major
    layout, measured maximum, pre-split halves) must be current afterwards: bitwise the output of a freshly built module that
    holds the updated values."""
    from glfusion_amd import ops
    from glfusion_amd.models.layers import Conv2d
    from glfusion_amd.optim import SGD
    ops.set_precision("f16x3")
    try:
        g = torch.Generator().manual_seed(5)
        conv = Conv2d(32, 40, 3, padding=1).to(DEV)
        x = torch.randn(3, 32, 15, 13, generator=g).to(DEV)
        with torch.no_grad():
            y0 = conv(x).clone()                                   # builds and registers the weight images
        opt = SGD(conv.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-4)
        for _ in range(2):
            conv.weight.grad = torch.randn(conv.weight.shape, generator=g).to(DEV)
            conv.bias.grad = torch.randn(conv.bias.shape, generator=g).to(DEV)
            opt.step()
        with torch.no_grad():
            y1 = conv(x).clone()
            fresh = Conv2d(32, 40, 3, padding=1).to(DEV)
            fresh.load_state_dict(conv.state_dict())
            y2 = fresh(x)
        assert not torch.equal(y0, y1)
        assert torch.equal(y1, y2)
    finally:
        ops.set_precision("f32")


def test_sgd_refuses_what_it_does_not_build():
    from glfusion_amd.optim import SGD
    p = torch.nn.Parameter(torch.zeros(4, 6, device=DEV).t())
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="glfusion_amd.optim.SGD: non-contiguous parameter"):
        SGD([p], lr=0.1).step()
    h = torch.nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))
    h.grad = torch.ones_like(h)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SGD([h], lr=0.1).step()
