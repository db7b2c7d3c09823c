"""GPU: the stem's input gradient (glf_stem7x7_dgrad / glf_s16_stem7x7_dgrad; early_fusion's stem reads a learned mix of the views'
images, so its input needs a gradient) against F.conv2d's own input gradient in float64 on the CPU.

Gate, element-wise: |got - want| <= (49 * 64 + 2) u sum |dy| |w|, u = 2^-24 -- every element is a sum of at most 49 * 64 products in
fp32, in four chains folded at the end; the bound holds for any order.  bf16 storage: the gradient handed in is bf16-representable, the
arithmetic is the same fp32, so the same bound."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24


def rnd(shape, seed):
    return 2.0 * torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 1.0


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("n,h,w,pad", [(1, 7, 7, 3), (2, 16, 16, 3), (2, 17, 33, 3), (1, 23, 9, 2), (3, 8, 21, 0)])
def test_stem_dgrad_against_float64(n, h, w, pad, prec):
    from glfusion_amd import ops
    ho, wo = h + 2 * pad - 6, w + 2 * pad - 6
    x = rnd((n, h, w, 1), 1)
    wt, b = rnd((64, 1, 7, 7), 2), rnd((64,), 3)
    dy = rnd((n, ho, wo, 64), 4).bfloat16().float()                       # representable in both storages
    x64 = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    F.conv2d(x64, wt.double(), b.double(), padding=pad).backward(dy.double().permute(0, 3, 1, 2))
    want = x64.grad.permute(0, 2, 3, 1)
    mag = torch.nn.grad.conv2d_input((n, 1, h, w), wt.double().abs(), dy.double().abs().permute(0, 3, 1, 2), padding=pad).permute(0, 2, 3, 1)
    xg = x.to(DEV).requires_grad_(True)
    wg, bg = wt.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    with ops.precision_scope(prec):
        y = ops.stem7x7(xg, wg, bg, pad)
        assert y.dtype == (torch.bfloat16 if prec == "bf16" else torch.float32) and tuple(y.shape) == (n, ho, wo, 64)
        y.backward(dy.to(DEV).to(y.dtype))
    torch.cuda.synchronize()
    got = xg.grad.cpu()
    assert tuple(got.shape) == (n, h, w, 1) and bool(torch.isfinite(got).all())
    err = (got.double() - want).abs()
    print(f"stem dgrad {prec} {n}x{h}x{w} pad {pad}: worst element at {float((err / ((49 * 64 + 2) * U * mag).clamp_min(1e-300)).max()):.3f} of its bound")
    assert bool((err <= (49 * 64 + 2) * U * mag).all())
    assert wg.grad is not None and bg.grad is not None                       # the weight gradient still comes with it


def test_stem_without_input_gradient_launches_no_dgrad(monkeypatch):
    from glfusion_amd import ops
    from glfusion_amd._lib import lib
    launched = []
    real = lib.load().glf_stem7x7_dgrad
    monkeypatch.setattr(lib.load(), "glf_stem7x7_dgrad", lambda *a: launched.append(1) or real(*a))
    x = rnd((1, 16, 16, 1), 5).to(DEV)
    wg = rnd((64, 1, 7, 7), 6).to(DEV).requires_grad_(True)
    ops.stem7x7(x, wg, None, 3).sum().backward()
    torch.cuda.synchronize()
    assert not launched and wg.grad is not None
