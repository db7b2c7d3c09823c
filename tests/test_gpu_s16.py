"""GPU: the 16-bit-storage mode (precision "bf16": BASELINE.json configs[2] / [4] -- bf16 activations, saved tensors and
activation gradients in HBM, fp32 master weights, fp32 accumulate; glfusion_amd.ops16, csrc/gemm_s16.hip, csrc/s16_ops.hip).

Three layers of evidence, each with its own stated tolerance:
  * kernels against torch on THE SAME bf16 inputs: what differs is one rounding of the result to bf16 (unit roundoff 2^-8: 8-bit significand, round-to-nearest-even) and the
    order of fp32 sums -- relative L2 <= 4e-3 for bf16 results, <= 1e-5 for fp32 results (weight gradients, statistics);
  * blocks (Bottleneck, DeepLabHead, TPAVIModule) against the oracle evaluated in float64: a few layers of bf16 rounding --
    output, input gradient and the median parameter gradient within 5e-2 relative L2, no tensor beyond 0.2;
  * the whole network: eval logits within 6e-2 of the largest logit and Dice within 2e-3 of the reference's fixture; train steps
    against the oracle in float64 with EVERY parameter gradient (encoders included) gated -- see
    test_s16_e2e_train_step_gradients_zero_mean_fixture for what fifty train-mode layers do to 8-bit mantissas and how the gate
    is built, and test_s16_e2e_train_step_vs_reference_kinkfree_fixture for the reference-pinned fixture.
This mode is NOT fp32-equivalent and is never reported as the fp32 headline (bench.py leg `config3_bf16`)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import glfusion_ref as orc   # the checker (tests only)
from test_gpu_s16_gemm import gate_interval   # per-element interval against float64

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _s16_mode():
    from glfusion_amd import ops
    ops.set_precision("bf16")
    yield
    ops.set_precision("f32")


def l2(a, b) -> float:
    a, b = torch.as_tensor(a).detach().float().cpu().double(), torch.as_tensor(b).detach().cpu().double()
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def rnd(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + shift).to(DEV)


# ----------------------------------------------------------------------------------------
# kernels vs torch on the same bf16 inputs
# ----------------------------------------------------------------------------------------
CONV_CASES = [
    # n, h, w, cin, cout, k, stride, pad, dil
    (2, 28, 28, 64, 64, 1, 1, 0, 1),
    (2, 28, 28, 64, 128, 3, 1, 1, 1),
    (2, 28, 28, 128, 64, 3, 1, 2, 2),
    (3, 28, 28, 64, 64, 3, 1, 12, 12),      # ASPP rate 12: region mode
    (3, 28, 28, 64, 192, 3, 1, 24, 24),     # ASPP rate 24: region mode
    (2, 28, 28, 64, 64, 3, 1, 36, 36),      # ASPP rate 36: the centre tap only
    (2, 55, 55, 64, 64, 3, 2, 1, 1),        # layer2 block 0: stride 2
    (2, 55, 55, 64, 128, 1, 2, 0, 1),       # its downsample
    (1, 30, 26, 128, 64, 3, 1, 4, 4),       # non-square map
]


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_s16_conv2d_fwd_dgrad_wgrad(case):
    from glfusion_amd import ops
    n, h, w, cin, cout, k, stride, pad, dil = case
    x = rnd((n, h, w, cin), 1).to(BF).requires_grad_(True)
    wt = (rnd((cout, cin, k, k), 2) / (cin * k * k) ** 0.5).requires_grad_(True)
    wq = wt.detach().to(BF).float()                                      # the kernels see bf16 weights
    sums = ops.stats_slot(cout, x.device)
    y = ops.conv2d(x, wt, None, stride, pad, dil, sums)
    assert y.dtype == BF
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    wr = wq.clone().requires_grad_(True)
    ref = F.conv2d(xr, wr, None, stride, pad, dil)
    assert l2(y, ref.permute(0, 2, 3, 1)) <= 4e-3
    # fused statistics: sums of the fp32 results before rounding
    assert l2(sums[0], ref.double().sum((0, 2, 3))) <= 1e-5 and l2(sums[1], (ref.double() ** 2).sum((0, 2, 3))) <= 1e-5
    dy = rnd(tuple(y.shape), 3).to(BF)
    y.backward(dy)
    ref.backward(dy.float().permute(0, 3, 1, 2))
    assert x.grad.dtype == BF and wt.grad.dtype == torch.float32
    assert l2(x.grad, xr.grad.permute(0, 2, 3, 1)) <= 4e-3
    assert l2(wt.grad, wr.grad) <= 1e-5
    # element by element against float64 on the same bf16 operands: the derived interval of tests/test_gpu_s16_gemm.py (evidence (b))
    x64 = x.detach().cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
    w64 = wq.cpu().double().requires_grad_(True)
    dy64 = dy.cpu().double().permute(0, 3, 1, 2)
    y64 = F.conv2d(x64, w64, None, stride, pad, dil)
    y64.backward(dy64)
    xa, wa = x64.detach().abs().requires_grad_(True), w64.detach().abs().requires_grad_(True)
    ya = F.conv2d(xa, wa, None, stride, pad, dil)
    ya.backward(dy64.abs())
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)
    gate_interval(y.detach().cpu(), nhwc(y64), nhwc(ya), cin * k * k, True, "y")
    gate_interval(x.grad.cpu(), nhwc(x64.grad), nhwc(xa.grad), cout * k * k, True, "x.grad")
    gate_interval(wt.grad.cpu(), w64.grad, wa.grad, int(y.numel()) // cout, False, "wt.grad")


def test_s16_conv_bias_and_narrow_head():
    """A conv with bias on the 16-bit kernels, and the 5- / 1-channel head logits (fp32 results through the exact kernels)."""
    from glfusion_amd import ops
    x = rnd((2, 28, 28, 256), 4).to(BF).requires_grad_(True)
    for cout in (64, 5, 1):
        wt = (rnd((cout, 256, 1, 1), 5) / 16).requires_grad_(True)
        b = rnd((cout,), 6).requires_grad_(True)
        y = ops.conv2d(x, wt, b, 1, 0, 1)
        assert y.dtype == (BF if cout == 64 else torch.float32)
        wq = wt.detach().to(BF).float() if cout == 64 else wt.detach()
        xr = x.detach().float().requires_grad_(True)
        wr, br = wq.clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        ref = F.conv2d(xr.permute(0, 3, 1, 2), wr, br).permute(0, 2, 3, 1)
        assert l2(y, ref) <= 4e-3
        dy = rnd(tuple(y.shape), 7).to(y.dtype)
        x.grad = None
        y.backward(dy)
        ref.backward(dy.float())
        assert l2(x.grad, xr.grad) <= 4e-3 and l2(wt.grad, wr.grad) <= 1e-4 and l2(b.grad, br.grad) <= 1e-5


@pytest.mark.parametrize("relu,with_res", [(True, False), (True, True), (False, False), (False, True)])
def test_s16_batchnorm_train_and_eval(relu, with_res):
    from glfusion_amd import ops
    from glfusion_amd.models.layers import BatchNorm2d
    c, shape = 128, (3, 17, 19, 128)
    bn = BatchNorm2d(c).to(DEV)
    ref = torch.nn.BatchNorm2d(c).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(rnd((c,), 8, 0.3, 1.0)); bn.bias.copy_(rnd((c,), 9, 0.5))
        ref.load_state_dict(bn.state_dict())
    x = rnd(shape, 10, 2.0, 0.7).to(BF).requires_grad_(True)
    res = rnd(shape, 11).to(BF).requires_grad_(True) if with_res else None
    y = ops.batch_norm_act(x, bn, relu, res)
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    rr = res.detach().float().permute(0, 3, 1, 2).requires_grad_(True) if with_res else None
    yr = ref(xr)
    if with_res:
        yr = yr + rr
    if relu:
        yr = torch.relu(yr)
    assert y.dtype == BF and l2(y, yr.permute(0, 2, 3, 1)) <= 4e-3
    dy = rnd(shape, 12).to(BF)
    y.backward(dy)
    # the backward ReLU mask is the sign of the value the kernel computed: compare through the same mask where the two differ by rounding
    yr.backward(dy.float().permute(0, 3, 1, 2))
    assert l2(x.grad, xr.grad.permute(0, 2, 3, 1)) <= 6e-3
    if with_res:
        assert l2(res.grad, rr.grad.permute(0, 2, 3, 1)) <= 6e-3
    assert l2(bn.weight.grad, ref.weight.grad) <= 2e-3 and l2(bn.bias.grad, ref.bias.grad) <= 2e-3
    assert l2(bn.running_mean, ref.running_mean) <= 1e-5 and l2(bn.running_var, ref.running_var) <= 1e-5
    assert int(bn.num_batches_tracked) == 1
    bn.eval(); ref.eval()
    with torch.no_grad():
        ye = ops.batch_norm_act(x.detach(), bn, relu, res.detach() if with_res else None)
        yre = ref(xr.detach())
        if with_res:
            yre = yre + rr.detach()
        if relu:
            yre = torch.relu(yre)
    assert l2(ye, yre.permute(0, 2, 3, 1)) <= 4e-3


def test_s16_lazy_fan_in_pair_equals_summed_gradient():
    """BatchNorm backward adds the two gradients of a block input while reading them (dy2) -- same result as adding first."""
    from glfusion_amd import ops, ops16
    from glfusion_amd.models.layers import BatchNorm2d
    c = 64
    bn = BatchNorm2d(c).to(DEV)
    x = rnd((2, 9, 9, c), 13).to(BF).requires_grad_(True)
    outs = []
    for lazy in (True, False):
        x.grad = None; bn.weight.grad = None; bn.bias.grad = None
        y = ops.batch_norm_act(x, bn, True)
        a, b = ops.fan_out(y, 2, lazy=lazy)
        (ops16.to_f32(a) * 2.0 + ops16.to_f32(b) * 3.0).sum().backward()
        outs.append((x.grad.clone(), bn.weight.grad.clone()))
    assert l2(outs[0][0], outs[1][0].float()) <= 4e-3 and l2(outs[0][1], outs[1][1]) <= 2e-3


def test_s16_pointwise_kernels():
    from glfusion_amd import ops, ops16
    # max-pool: values and gradient routing equal to ATen's on the same data
    x = rnd((2, 55, 55, 64), 14).to(BF).requires_grad_(True)
    y = ops.maxpool3x3s2(x)
    xr = x.detach().float().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.max_pool2d(xr, 3, 2, 1)
    assert torch.equal(y.float(), yr.permute(0, 2, 3, 1).contiguous())            # a selection: bit-exact
    dy = rnd(tuple(y.shape), 15).to(BF)
    y.backward(dy)
    yr.backward(dy.float().permute(0, 3, 1, 2))
    assert l2(x.grad, xr.grad.permute(0, 2, 3, 1)) <= 4e-3
    # global average pool + broadcast (ASPP pooled branch)
    x = rnd((3, 7, 9, 128), 16).to(BF).requires_grad_(True)
    p = ops.global_avgpool(x)                      # fp32: the pooled branch stays fp32 up to its broadcast
    b = ops.broadcast_hw(p, 7, 9)
    assert p.dtype == torch.float32 and b.dtype == BF
    assert l2(p, x.detach().float().mean((1, 2), keepdim=True)) <= 1e-6
    assert l2(b, p.detach().expand(3, 7, 9, 128)) <= 4e-3
    g = rnd((3, 7, 9, 128), 17).to(BF)
    b.backward(g)
    assert l2(x.grad, g.float().sum((1, 2), keepdim=True).expand(3, 7, 9, 128) / 63.0) <= 4e-3
    # dropout: kept elements scaled by 1 / (1 - p), the same mask in forward and backward
    x = rnd((4, 8, 8, 64), 18, 1.0, 3.0).to(BF).requires_grad_(True)
    y = ops.dropout(x, 0.5, True)
    keep = y.detach().float() != 0
    assert 0.4 < float(keep.float().mean()) < 0.6
    assert l2(y.detach().float()[keep], 2.0 * x.detach().float()[keep]) <= 4e-3
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad.float() != 0, keep)
    # relu / axpby
    x = rnd((2, 5, 5, 64), 19).to(BF).requires_grad_(True)
    y = ops.relu(x)
    assert torch.equal(y.float(), torch.relu(x.detach().float()))
    y.backward(torch.ones_like(y))
    assert torch.equal(x.grad.float(), (x.detach().float() > 0).float())
    a, b = rnd((2, 5, 5, 64), 20).to(BF), rnd((2, 5, 5, 64), 21).to(BF)
    assert l2(ops.axpby(a, b, 1.0, -1.0), a.float() - b.float()) <= 4e-3
    # casts round-trip
    f = rnd((2, 5, 5, 64), 22)
    assert torch.equal(ops16.to_bf16(f), f.to(BF)) and torch.equal(ops16.to_f32(f.to(BF)), f.to(BF).float())
    # 16-bit transpose
    m = rnd((3, 96, 160), 23).to(BF)
    assert torch.equal(ops16.transpose16(m, 96, 160, 3).view(3, 160, 96), m.transpose(1, 2).contiguous())


def test_s16_gate_stack_add_views():
    from glfusion_amd import ops
    n, h, w, c = 2, 6, 7, 128
    f = rnd((n, h, w, c), 24).to(BF).requires_grad_(True)
    cls = rnd((n, h, w, 5), 25).requires_grad_(True)
    ctr = rnd((n, h, w, 1), 26).requires_grad_(True)
    y = ops.local_gate(cls, ctr, f, 20.0)
    fr, cr, tr = f.detach().float().requires_grad_(True), cls.detach().clone().requires_grad_(True), ctr.detach().clone().requires_grad_(True)
    a = torch.sigmoid(20.0 * torch.sigmoid(cr).max(-1, keepdim=True).values * torch.sigmoid(tr))
    yr = fr * a
    assert l2(y, yr) <= 4e-3
    g = rnd((n, h, w, c), 27).to(BF)
    y.backward(g)
    yr.backward(g.float())
    assert l2(f.grad, fr.grad) <= 4e-3 and l2(cls.grad, cr.grad) <= 2e-3 and l2(ctr.grad, tr.grad) <= 2e-3
    xs = [rnd((n, h, w, c), 30 + i).to(BF).requires_grad_(True) for i in range(3)]
    st = ops.stack_views(xs)
    assert torch.equal(st, torch.stack([t.detach() for t in xs], 1))
    g2, l2_ = rnd((n, 3, h, w, c), 40).to(BF).requires_grad_(True), rnd((n, 3, h, w, c), 41).to(BF).requires_grad_(True)
    outs = ops.add_views(g2, l2_)
    for i, o in enumerate(outs):
        assert l2(o, g2.detach().float()[:, i] + l2_.detach().float()[:, i]) <= 4e-3
    (st.float().sum() * 1.0).backward()
    assert all(torch.equal(t.grad.float(), torch.ones_like(t.grad).float()) for t in xs)


def test_s16_stem():
    from glfusion_amd import ops
    x = torch.rand(2, 40, 36, 1, device=DEV)
    w = (rnd((64, 1, 7, 7), 50) / 7).requires_grad_(True)
    b = rnd((64,), 51).requires_grad_(True)
    y = ops.stem7x7(x, w, b, 2)
    wr, br = w.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = F.conv2d(x.permute(0, 3, 1, 2), wr, br, 1, 2)
    assert y.dtype == BF and l2(y, yr.permute(0, 2, 3, 1)) <= 4e-3
    dy = rnd(tuple(y.shape), 52).to(BF)
    y.backward(dy)
    yr.backward(dy.float().permute(0, 3, 1, 2))
    assert l2(w.grad, wr.grad) <= 1e-5 and l2(b.grad, br.grad) <= 1e-5


# ----------------------------------------------------------------------------------------
# blocks vs the oracle in float64
# ----------------------------------------------------------------------------------------
def zero_mean_kinkfree_fill(module, seed: int, offset: float = 3.0) -> None:
    """The fixture weights of the gradient tests of this mode: torch's default (zero-mean, kaiming) initialisation under a seed,
    then every BatchNorm2d beta at +-offset by channel parity and gamma in [0.9, 1.1] -- no ReLU input comes within bf16
    rounding distance of zero (3 standard deviations), so gradients are smooth in the arithmetic, as with oracle.kinkfree_fill;
    unlike it the conv weights have ZERO mean: a conv output's mean stays of the order of its spread.  (With the closed-form
    fill's positive weights on positive activations a K = 256 conv output has a mean ~40x its standard deviation, and storing
    THAT in 8 mantissa bits throws away 5 of them -- a property of that fixture, not of trained networks.)"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
                if isinstance(m, torch.nn.Conv2d) and m.out_channels == 1 and m.bias is not None:
                    m.weight.mul_(0.02); m.bias.fill_(-3.0)          # centre-ness logit: keeps the local gate away from saturation
            elif isinstance(m, torch.nn.BatchNorm2d):
                c = m.num_features
                m.bias.copy_(torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0) * offset)
                m.weight.copy_(0.9 + 0.2 * torch.rand(c, generator=g))
            elif isinstance(m, torch.nn.BatchNorm3d):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))
            elif isinstance(m, torch.nn.LayerNorm):
                m.weight.copy_(1.0 + 0.1 * torch.randn(m.weight.shape, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))



def _block_check(hip_mod, ref_mod, x_nchw, tol, fwd=None, what=""):
    """hip_mod.forward_nhwc on the bf16 input vs ref_mod (float64) on the fp32 input: output and every gradient within tol."""
    from glfusion_amd import ops, ops16
    ref_mod.load_state_dict(hip_mod.state_dict(), strict=True)
    orc.set_dropout(hip_mod, 0.0); orc.set_dropout(ref_mod, 0.0)
    ref_mod = ref_mod.double().train()
    hip_mod = hip_mod.to(DEV).train()
    x = x_nchw.to(DEV).requires_grad_(True)
    xh = ops16.to_bf16(ops.to_nhwc(x) if x.dim() == 4 else x.permute(0, 2, 3, 4, 1).contiguous())
    y = (fwd or (lambda m, t: m.forward_nhwc(t)))(hip_mod, xh)
    y = ops16.to_f32(y) if y.dtype == BF else y
    xr = x_nchw.double().requires_grad_(True)
    yr = ref_mod(xr)
    yr = yr[0] if isinstance(yr, tuple) else yr
    yr_l = yr.permute(0, 2, 3, 1) if yr.dim() == 4 else yr.permute(0, 2, 3, 4, 1)
    e_out = l2(y, yr_l)
    dy = orc.closed_form_tensor(tuple(yr_l.shape), 77, -1.0, 1.0)
    y.backward(dy.to(DEV))
    yr_l.backward(dy.double())
    errs = {"out": e_out, "dx": l2(x.grad, xr.grad)}
    want = dict(ref_mod.named_parameters())
    for k, p in hip_mod.named_parameters():
        if want[k].grad is None:
            continue
        if float(want[k].grad.norm()) < 1e-3 * max(float(q.grad.norm()) for q in want.values() if q.grad is not None):
            continue                                  # structurally ~zero (a bias in front of a train-mode BatchNorm)
        errs[k] = l2(p.grad, want[k].grad)
    worst = max(errs.items(), key=lambda kv: kv[1])
    med = float(np.median(list(errs.values())))
    print(f"s16 {what}: out {e_out:.2e}, dx {errs['dx']:.2e}, median {med:.2e}, worst {worst[0]} {worst[1]:.2e}")
    # output and input gradient within tol, the median over all tensors within tol, no single tensor beyond 4 x tol (BatchNorm bias
    # gradients are sums over all rows that largely cancel: the few worst tensors are always those)
    assert e_out <= tol and errs["dx"] <= tol and med <= tol and worst[1] <= 4 * tol, errs
    return errs


def test_s16_bottleneck_block_vs_oracle():
    from glfusion_amd.models import resnet as hip_resnet
    from glfusion_amd.models.layers import BatchNorm2d, Conv2d
    for inplanes, planes, stride, dil in ((256, 64, 1, 1), (256, 128, 2, 1), (512, 128, 1, 2)):
        down = rdown = None
        if stride != 1 or inplanes != planes * 4:
            down = torch.nn.Sequential(Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False), BatchNorm2d(planes * 4))
            rdown = torch.nn.Sequential(torch.nn.Conv2d(inplanes, planes * 4, kernel_size=1, stride=stride, bias=False), torch.nn.BatchNorm2d(planes * 4))
        blk = hip_resnet.Bottleneck(inplanes, planes, stride, down, dil)
        zero_mean_kinkfree_fill(blk, 31)
        ref = orc.Bottleneck(inplanes, planes, stride, rdown, dil)
        x = torch.randn(4, inplanes, 28, 28, generator=torch.Generator().manual_seed(311)).abs()
        _block_check(blk, ref, x, 5e-2, what=f"bottleneck {inplanes}/{planes}/s{stride}/d{dil}")


def test_s16_deeplab_head_vs_oracle():
    from glfusion_amd.models.deeplabv3 import DeepLabHead
    head = DeepLabHead(128, 5)
    zero_mean_kinkfree_fill(head, 41)
    ref = orc.DeepLabHead(128, 5)
    x = torch.randn(8, 128, 28, 28, generator=torch.Generator().manual_seed(411)).abs()
    _block_check(head, ref, x, 5e-2, what="DeepLabHead(128, 5)")


def test_s16_tpavi_block_vs_oracle():
    from glfusion_amd.models.ours import TPAVIModule
    mod = TPAVIModule(in_channels=128, mode="dot")
    zero_mean_kinkfree_fill(mod, 51)
    ref = orc.TPAVIModule(in_channels=128, mode="dot")
    x = torch.randn(3, 128, 3, 10, 12, generator=torch.Generator().manual_seed(511))          # [N, C, V, h, w]
    _block_check(mod, ref, x, 5e-2, fwd=lambda m, t: m.forward_nvhwc(t), what="TPAVIModule(128)")


@pytest.mark.parametrize("training", [True, False])
def test_s16_tpavi_single_call_equals_composed_sequence(training, monkeypatch):
    """glf_s16_tpavi_fwd / _bwd (one C call per direction, include/glfusion.h) against the same block composed from the
    individual entry points by fusion16.Tpavi16Fn: the same launches, so every output, buffer update and gradient bit for bit."""
    from glfusion_amd import ops16
    from glfusion_amd.models.ours import TPAVIModule
    res = []
    for block_calls in (True, False):
        monkeypatch.setattr(ops16, "BLOCK_CALLS", block_calls)
        mod = TPAVIModule(in_channels=256, mode="dot")
        zero_mean_kinkfree_fill(mod, 52)
        mod = mod.to(DEV).train(training)
        x = torch.randn(2, 3, 20, 24, 256, generator=torch.Generator().manual_seed(512)).to(DEV).to(BF).requires_grad_(True)
        z = mod.forward_nvhwc(x)
        z.backward(torch.randn(z.shape, generator=torch.Generator().manual_seed(513)).to(DEV).to(BF))
        torch.cuda.synchronize()
        res.append((z.detach(), x.grad, {k: p.grad for k, p in mod.named_parameters()}, dict(mod.named_buffers())))
    (z1, dx1, g1, b1), (z0, dx0, g0, b0) = res
    assert torch.equal(z1, z0) and torch.equal(dx1, dx0)
    for k in g0:
        assert (g0[k] is None and g1[k] is None) or torch.equal(g1[k], g0[k]), k
    for k in b0:
        assert torch.equal(b1[k], b0[k]), k


def test_s16_tpavi_single_call_argument_checks():
    import ctypes as C
    from glfusion_amd._lib import TpaviParams, lib
    tp = TpaviParams(2, 64, 128, 64, 1, 1e-5, 0.1, 1e-5)
    assert lib.glf_s16_tpavi_workspace_bytes(C.byref(tp), 1) > lib.glf_s16_tpavi_workspace_bytes(C.byref(tp), 0) > 0
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    args_f = [p] * 21
    assert lib.glf_s16_tpavi_fwd(*args_f, C.byref(tp), p, 16, None) == -3                 # GLF_ERR_WORKSPACE: too small
    assert b"workspace" in lib.glf_last_error()
    bad = TpaviParams(2, 64, 100, 64, 1, 1e-5, 0.1, 1e-5)
    assert lib.glf_s16_tpavi_fwd(*args_f, C.byref(bad), p, 1 << 16, None) == -2           # GLF_ERR_UNSUPPORTED: C % 64
    args_f[0] = None
    assert lib.glf_s16_tpavi_fwd(*args_f, C.byref(tp), p, 1 << 16, None) == -5            # GLF_ERR_NULL


# ----------------------------------------------------------------------------------------
# the whole network vs the reference's fixtures
# ----------------------------------------------------------------------------------------
def test_s16_e2e_eval_vs_golden(golden_dir):
    """BASELINE config 3 on the reference's own eval fixture (tests/golden/e2e_eval_c2.npz: the reference's classes, closed-form
    weights): logits within 6e-2 of the largest logit, Dice within 2e-3 (fp32 modes: 1e-4 / 1e-4)."""
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    g = np.load(os.path.join(golden_dir, "e2e_eval_c2.npz"))
    views, n = ["1", "3", "4"], 2
    model = Global_and_Local(views)
    orc.closed_form_fill(model, salt=1)
    model = model.to(DEV).eval()
    imgs = {v: t.to(DEV) for v, t in orc.closed_form_images(views, n).items()}
    tgts = orc.closed_form_targets(views, n)
    with torch.no_grad():
        mask, mask_bb, f4g, f4l = model(imgs)
    for v in views:
        assert mask[v].dtype == torch.float32 and f4g[v].dtype == BF
        for got, key in ((mask[v], f"mask:{v}"), (mask_bb[v], f"mask_bb:{v}")):
            ref = torch.from_numpy(g[key])
            err = float((got.cpu() - ref).abs().max()) / float(ref.abs().max())
            assert err <= 6e-2, (key, err)
        dice = ops.overlap_metrics_from_counts(ops.overlap_counts(mask[v], tgts[v].to(DEV)))
        assert abs(dice[1] - float(g[f"dice:{v}"][1])) <= 2e-3, (v, dice[1], float(g[f"dice:{v}"][1]))


def _grad_rows(model, want, scale):
    rows = []
    for name, p in model.named_parameters():
        if name not in want:
            assert p.grad is None, name
            continue
        w = want[name]
        if float(w.norm()) <= 1e-2 * scale[name.split(".")[0]]:
            continue
        got = p.grad.detach().cpu().double()
        proj = float((got * w).sum() / (w * w).sum())
        cos = float((got * w).sum() / (got.norm() * w.norm()))
        rows.append((float((got - w).norm() / w.norm()), cos, proj, name, w.numel()))
    rows.sort(reverse=True)
    return rows


def test_s16_e2e_train_step_gradients_zero_mean_fixture():
    """A full train step of Global_and_Local (2 views x 4 frames, zero_mean_kinkfree_fill, Dropout off) against the oracle evaluated
    in float64, EVERY parameter gradient of non-negligible norm gated, encoders included:
      * relative L2 <= 0.5, cosine >= 0.85, projection <g16, g> / <g, g> in [0.8, 1.2] (tensors of >= 1024 elements): no systematic
        scale error -- a wrong factor, a dropped term or a mis-routed tensor moves the projection far outside, rounding noise does
        not (it is uncorrelated with g);
      * the deviation is the mantissa's: per parameter group the median relative L2 under bf16 STORAGE (8 bits) stays within 16x
        that of the same step under fp16 OPERANDS (precision "f16": 11 bits, fp32 storage) -- measured 7-8x, i.e. 2^3.
    Measured here: 0.2 - 0.3 relative L2 (cosine 0.93 - 0.98) on the encoders and fusion blocks, 0.04 on the classifier heads;
    the fp32-equivalent precision sits at 3e-5 on the same fixture.  That is what fifty train-mode BatchNorm layers make of
    2^-9 relative rounding per stored tensor; it is noise around the true gradient, not a bias."""
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    views, n = ["1", "3"], 4
    model0 = Global_and_Local(views)
    zero_mean_kinkfree_fill(model0, 7)
    orc.set_dropout(model0, 0.0)
    sd = {k: v.clone() for k, v in model0.state_dict().items()}
    ref = orc.Global_and_Local(views)
    ref.load_state_dict(sd, strict=True)
    orc.set_dropout(ref, 0.0)
    ref = ref.double().train()
    imgs, tgts = orc.varied_images(views, n), orc.closed_form_targets(views, n)
    pred = ref({v: imgs[v].double() for v in views})[0]
    loss_ref = sum(F.binary_cross_entropy_with_logits(pred[v], tgts[v].double(), reduction="sum") for v in views)
    loss_ref.backward()
    want = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
    scale = {}
    for k, w in want.items():
        scale[k.split(".")[0]] = max(scale.get(k.split(".")[0], 0.0), float(w.norm()))
    med = {}
    for prec in ("bf16", "f16"):
        ops.set_precision(prec)
        model = Global_and_Local(views)
        model.load_state_dict(sd, strict=True)
        orc.set_dropout(model, 0.0)
        model = model.to(DEV).train()
        out = model({v: imgs[v].to(DEV) for v in views})[0]
        loss = sum(ops.bce_with_logits_sum(out[v], tgts[v].to(DEV)) for v in views)
        loss.backward()
        assert abs(float(loss.detach()) - float(loss_ref)) <= 1e-3 * float(loss_ref)
        rows = _grad_rows(model, want, scale)
        by = {}
        for rel, cos, proj, name, numel in rows:
            by.setdefault(name.split(".")[0], []).append(rel)
        med[prec] = {k: float(np.median(v)) for k, v in by.items()}
        if prec == "bf16":
            print("s16 zero-mean fixture: worst relative L2", [f"{r[3]} {r[0]:.2f}" for r in rows[:3]], " lowest cosine", min(r[1] for r in rows),
                  " projection range", min(r[2] for r in rows if r[4] >= 1024), max(r[2] for r in rows if r[4] >= 1024))
            assert len(rows) > 200
            for rel, cos, proj, name, numel in rows:
                assert rel <= 0.5 and cos >= 0.85, (name, rel, cos)
                if numel >= 1024:
                    assert 0.8 <= proj <= 1.2, (name, proj)
    ops.set_precision("bf16")
    print("s16 zero-mean fixture: median relative L2 per group, bf16 storage vs fp16 operands:", {k: (round(med["bf16"][k], 4), round(med["f16"][k], 4)) for k in med["bf16"]})
    for k in med["bf16"]:
        assert med["bf16"][k] <= 16.0 * med["f16"][k] + 0.02, (k, med["bf16"][k], med["f16"][k])


def test_s16_e2e_train_step_vs_reference_kinkfree_fixture(golden_dir):
    """The reference-pinned kink-free train step (tests/golden/e2e_train_kinkfree.npz; truth = the oracle in float64, itself
    checked against the reference's fp64 run) under 16-bit storage: loss within 1e-3, logits within 5e-2 relative L2, and the
    parameter gradients PER GROUP (init_block, layer1-4, classifier, the two fusion blocks -- encoders included): median relative
    L2 <= 1.0, median cosine >= 0.5, and the group's projection sum <g16, g> / sum <g, g> in [0.35, 1.5] (measured 0.49 - 1.0,
    falling with depth: on this fixture reduced precision attenuates the gradient -- fp16 OPERANDS on the validated fp32-storage
    kernels show the same deficit at an eighth of the size, 0.95 - 0.97, i.e. it scales with the mantissa, and the zero-mean
    fixture above, where the per-tensor projection gate is [0.8, 1.2], does not show it).
    This fixture is hostile to ANY 8-bit-mantissa storage: its closed-form weights are positive and its activations sit at
    +-6 +- 1, so a K = 256 conv output carries a mean ~40x its standard deviation into bf16 (zero_mean_kinkfree_fill explains),
    and single tensors move by tens of per cent between two runs that differ only in the order of a few atomics -- which is why
    the gate here is per group; the per-tensor gates are in the zero-mean test above and in the block tests.
    Measured: group medians 0.35 - 0.57 on the encoders (cosine 0.65 - 0.8); fp16 operands (11 bits) on the same step: 0.10 - 0.19.
    The centre-ness heads are reported, not gated, on this fixture: they get their gradient through the gate sigmoid(20 m c) from
    a 1-channel logit whose gradient is a strongly cancelling sum here (projection 2 - 8 on the head's last layers; fp16 operands:
    1.4 on the same tensors, same direction); the zero-mean test gates them per tensor."""
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    from test_gpu_model import _kinkfree_truth
    t = _kinkfree_truth(golden_dir)
    views, n = t["views"], t["n"]
    model = Global_and_Local(views)
    orc.kinkfree_fill(model, salt=21)
    orc.set_dropout(model, 0.0)
    model = model.to(DEV).train()
    pred = model({v: t["imgs"][v].to(DEV) for v in views})[0]
    loss = sum(ops.bce_with_logits_sum(pred[v], t["tgts"][v].to(DEV)) for v in views)
    loss.backward()
    assert abs(float(loss.detach()) - t["loss"]) <= 1e-3 * abs(t["loss"])
    for v in views:
        assert l2(pred[v], t["pred"][v]) <= 5e-2
    rows = _grad_rows(model, t["grads"], t["scale"])
    assert len(rows) > 150
    groups = {}
    for rel, cos, proj, name, numel in rows:
        g = groups.setdefault(name.split(".")[0], {"rel": [], "cos": [], "num": 0.0, "den": 0.0})
        w = t["grads"][name]
        g["rel"].append(rel); g["cos"].append(cos)
        g["num"] += proj * float((w * w).sum()); g["den"] += float((w * w).sum())
    report = {k: (round(float(np.median(g["rel"])), 3), round(float(np.median(g["cos"])), 3), round(g["num"] / g["den"], 3)) for k, g in groups.items()}
    print("s16 reference kink-free fixture: per group (median relative L2, median cosine, projection):", report)
    for k, (rel, cos, proj) in report.items():
        if k == "centerness":
            continue
        assert rel <= 1.0 and cos >= 0.5 and 0.35 <= proj <= 1.5, (k, rel, cos, proj)


def test_s16_config5_full_clip_T32_on_one_gpu():
    """BASELINE.json configs[4] ("bf16 ... long-sequence cross-view attention at the HBM limit") at its FULL per-GPU size under
    16-bit storage: one clip of 5 views x 32 frames x 224 x 224 (L = 15 680 positions per frame).  Size-independent checks, as in
    tests/test_gpu_model.py::test_config5_full_clip_T32_on_one_gpu: (a) the eval forward over 32 frames equals two 16-frame forwards
    (frames are independent under running statistics: the bf16 fusion features match bit for bit, the fp32 logits -- the 5-channel
    output conv runs on the exact-fp32 kernels, whose tiling depends on the row count -- to 1e-5) and the SUM loss adds up; (b) the train step is finite and every live parameter gets a finite, non-zero-norm gradient; (c) the step's peak
    allocation stays under 130 GB (fp32 storage: 230 GB with retained operand images, 183 GB without)."""
    import gc
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    views, T = ["1", "2", "3", "4", "5"], 32
    # what earlier tests of the same process still hold (models kept alive by reference cycles, retained operand images, pools) is not
    # this step's footprint: the peak is taken relative to the allocation level at the start of the test
    gc.collect()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    model = Global_and_Local(views)
    orc.closed_form_fill(model, salt=4)
    model = model.to(DEV)
    g = torch.Generator(device=DEV).manual_seed(5)
    imgs = {v: torch.rand(T, 1, 224, 224, device=DEV, generator=g) for v in views}
    tgts = {v: (torch.rand(T, 5, 224, 224, device=DEV, generator=g) < 0.3).float() for v in views}
    try:
        model.eval()
        with torch.no_grad():
            full, _, full_g, _ = model(imgs)
            l_full = sum(float(ops.bce_with_logits_sum(full[v], tgts[v])) for v in views)
            l_halves = 0.0
            for lo, hi in ((0, 16), (16, 32)):
                part, _, part_g, _ = model({v: t[lo:hi] for v, t in imgs.items()})
                for v in views:
                    assert torch.equal(part_g[v], full_g[v][lo:hi]), (v, lo)
                    assert float((part[v] - full[v][lo:hi]).abs().max()) <= 1e-5 * max(1.0, float(full[v].abs().max())), (v, lo)
                    l_halves += float(ops.bce_with_logits_sum(part[v], tgts[v][lo:hi]))
            assert abs(l_full - l_halves) <= 1e-6 * abs(l_full)
            del full, part, full_g, part_g
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        model.train()
        pred = model(imgs)[0]
        loss = sum(ops.bce_with_logits_sum(pred[v], tgts[v]) for v in views)
        loss.backward()
        torch.cuda.synchronize()
        lv = float(loss.detach())
        assert lv == lv and abs(lv) < 1e13
        live = {n for n, p in model.named_parameters() if p.grad is not None}
        assert len(live) > 1000 and not any(n.startswith("network.") or ".align_channel." in n for n in live)
        for n, p in model.named_parameters():
            if p.grad is not None:
                assert bool(torch.isfinite(p.grad).all()), n
        assert float(model.layer4["3"][2].conv3.weight.grad.abs().sum()) > 0 and float(model.global_attn.theta.weight.grad.abs().sum()) > 0
        peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
        print(f"s16 config 5, one clip (5 views x 32 x 224^2) on one GPU: loss {lv:.1f}, peak allocation {peak:.0f} GB "
              f"(+ {base / 2 ** 30:.0f} GB held by earlier tests of this process)")
        assert peak < 130
    finally:
        del model, imgs, tgts
        torch.cuda.empty_cache()
