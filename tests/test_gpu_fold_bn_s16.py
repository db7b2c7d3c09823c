"""GPU: opt-in folded-BatchNorm inference under 16-bit storage (ops.set_fold_bn_s16; glf_s16_fold_bn, glf_s16_gemm_nt_epilogue):
kernel-level accuracy against float64 with a torch emulation of the same roundings as yardstick, the mean-dominated channel, the fold
kernel bit for bit, write discipline, the epilogue-off identity, staleness of the folded images, no change of behaviour off the path,
the full model against the reference's golden outputs, hipGraph capture and the Trainer switch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import glfusion_ref as orc   # the checker (tests only)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NAN_BITS = 0x7fc1                        # a bf16 NaN pattern no kernel produces: what was never written keeps it


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    from glfusion_amd import ops
    yield
    ops.set_fold_bn(False)
    ops.set_fold_bn_s16(False)
    ops.set_precision("f32")


# ------------------------------------------------------------------------------------------------ helpers
def _bf16_rne(x64):
    """float64 -> bf16, ONE rounding to nearest even, as bit arithmetic on the double (torch's own float64 -> bfloat16 cast goes
    through fp32: two roundings).  Returns the bf16 tensor; every non-zero value must be a normal bf16 number."""
    u = x64.contiguous().view(torch.int64)
    sign = (u >> 48) & 0x8000
    mag = u & 0x7fffffffffffffff
    r = (mag + 0xfffffffffff + ((mag >> 45) & 1)) >> 45          # double exponent | 7 mantissa bits, the carry included
    bits = torch.where(mag == 0, torch.zeros_like(r), r - ((1023 - 127) << 7))
    assert bool(((bits == 0) | ((bits >= 0x80) & (bits < 0x7f80))).all()), "value outside the normal bf16 range"
    bits = sign | bits
    return torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(BF)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int16, device=DEV).view(BF)


def _bn_fill(bn, seed, spread):
    """As tests/test_gpu_fold_bn.py: gamma in [0.5, 1.5] with a negative one at every 7th channel, running_var over 1e-2 ... 1e2."""
    g = torch.Generator().manual_seed(seed)
    c = bn.num_features
    gamma = 0.5 + torch.rand(c, generator=g)
    gamma[::7] *= -1.0
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g) * spread)
        bn.running_var.copy_(10.0 ** (torch.rand(c, generator=g) * 4.0 - 2.0))


def _conv_bn(cin, cout, k, stride, pad, dil, seed, bias=False):
    from glfusion_amd.models.layers import BatchNorm2d, Conv2d
    torch.manual_seed(seed)
    conv = Conv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5)      # zero mean, conv output spread ~ 1
    bn = BatchNorm2d(cout)
    _bn_fill(bn, seed + 1, 1.0)
    return conv.to(DEV), bn.to(DEV).eval()


def _conv64(x64_nhwc, w64_oihw, stride, pad, dil):
    """float64 convolution on the device (im2col + matmul): [n, ho, wo, cout]."""
    x = x64_nhwc.permute(0, 3, 1, 2)
    n = x.shape[0]
    cout, cin, k, _ = w64_oihw.shape
    ho = (x.shape[2] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (x.shape[3] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    cols = F.unfold(x, k, dilation=dil, padding=pad, stride=stride)
    y = torch.matmul(w64_oihw.reshape(cout, -1), cols)
    return y.reshape(n, cout, ho, wo).permute(0, 2, 3, 1)


def _scale64(bn):
    eps = float(np.float32(bn.eps))                                                 # the C ABI takes eps as a float
    return bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + eps)


def _truth64(x, conv, bn, stride, pad, dil, relu, residual):
    """conv -> eval BatchNorm -> (+ residual) -> (ReLU) in float64 from the UNFOLDED fp32 parameters and the bf16 input as it is."""
    y = _conv64(x.double(), conv.weight.detach().double(), stride, pad, dil)
    y = (y - bn.running_mean.double()) * _scale64(bn) + bn.bias.detach().double()
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


def _emulation(x, conv, bn, stride, pad, dil, relu, residual):
    """The yardstick (as in tests/test_gpu_s16_attn.py): the same roundings and nothing else.  W' = W * s rounded to bf16 once from the
    double product, the contraction in float64, the fp32 shift and the residual added, ReLU, ONE rounding to bf16."""
    s = _scale64(bn)
    wf = _bf16_rne(conv.weight.detach().double() * s[:, None, None, None]).double()
    b = conv.bias.detach().double() if conv.bias is not None else 0.0
    shift = (bn.bias.detach().double() + (b - bn.running_mean.double()) * s).float().double()
    y = _conv64(x.double(), wf, stride, pad, dil) + shift
    if residual is not None:
        y = y + residual.double()
    return _bf16_rne(torch.relu(y) if relu else y)


def _rel(a, b):
    a, b = a.detach().double(), b.detach()
    return float((a - b).norm() / b.norm())


def _fold_direct(conv, bn):
    """(tap-major folded bf16 weights, fp32 shift) through glf_s16_fold_bn itself."""
    from glfusion_amd import ops
    from glfusion_amd._lib import check, lib
    cout, cin, k, _ = conv.weight.shape
    wt = ops.tap_major(conv.weight)
    wf = _nan_filled(k * k, cout, cin)
    shift = torch.full((cout,), float("nan"), device=DEV)
    check(lib.glf_s16_fold_bn(ops._p(wt), ops._p(conv.bias.detach()) if conv.bias is not None else None, ops._p(bn.weight.detach()),
                              ops._p(bn.bias.detach()), ops._p(bn.running_mean), ops._p(bn.running_var), float(bn.eps), ops._p(wf), ops._p(shift),
                              k * k, cout, cin, ops._stream()), "s16_fold_bn")
    return wf, shift


def _gparams(M, N, K, ldc, geo=None, mask=1, rect=0):
    from glfusion_amd._lib import GemmParams
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, K, K, ldc
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = geo if geo is not None else (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.taps = p.kh * p.kw
    p.tap_mask, p.tap_stride_b, p.gather, p.rect = mask, N * K, 1 if geo is not None else 0, rect
    p.batch, p.alpha, p.split, p.c_dtype = 1, 1.0, 1, 1                             # GLF_DT_BF16
    return p


def _epilogue_call(A, B, Cm, p, shift, residual=None, ld_res=0, relu=0):
    """glf_s16_gemm_nt_epilogue at the C ABI."""
    from glfusion_amd import ops
    from glfusion_amd._lib import S16GemmEpilogue, check, lib
    e = S16GemmEpilogue()
    e.shift, e.residual, e.ld_res, e.relu = shift.data_ptr(), residual.data_ptr() if residual is not None else None, ld_res, int(relu)
    check(lib.glf_s16_gemm_nt_epilogue(ops._p(A), ops._p(B), ops._p(Cm), C.byref(p), C.byref(e), ops._stream()), "s16_gemm_nt_epilogue")
    torch.cuda.synchronize()


CASES = {
    # name: (n, h, w, cin, cout, k, stride, pad, dil, relu, residual, plan rect)
    "a_1x1_res_relu": (2, 14, 14, 64, 256, 1, 1, 0, 1, True, True, 0),          # M = 392: ragged second row tile
    "b_3x3_s2_relu": (2, 17, 17, 128, 128, 3, 2, 1, 1, True, False, 0),         # gather, stride 2, odd map
    "c_3x3_dil2_identity": (2, 14, 14, 256, 256, 3, 1, 2, 2, False, False, 0),  # identity, no residual
    "d_3x3_dil12_region_relu": (1, 28, 28, 512, 256, 3, 1, 12, 12, True, False, 2),   # region mode, TK = 64
    "e_1x1_shift_only": (2, 9, 11, 256, 64, 1, 1, 0, 1, False, False, 0),       # the 64-wide tile
}


def _case(name, seed=None):
    n, h, w, cin, cout, k, stride, pad, dil, relu, has_res, want_rect = CASES[name]
    conv, bn = _conv_bn(cin, cout, k, stride, pad, dil, seed=len(name) if seed is None else seed)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, h, w, cin, generator=g).to(DEV).to(BF)
    ho = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn(n, ho, wo, cout, generator=g).to(DEV).to(BF) if has_res else None
    return conv, bn, x, res, (n, h, w, ho, wo, k, k, stride, pad, dil)


def _plan(x, conv, bn, stride, pad, dil):
    from glfusion_amd import ops, ops16
    ops.set_fold_bn_s16(True)
    with ops.precision_scope("bf16"), torch.no_grad():
        plan = ops16.fold_plan16(x, conv.weight, bn, stride, pad, dil)
    ops.set_fold_bn_s16(False)
    assert plan is not None
    return plan


def _folded_vs_float64(name, conv, bn, x, res, geo):
    """Runs the folded layer through the C entry points into a NaN-filled output; returns (kernel, emulation, unfolded) errors."""
    from glfusion_amd import ops
    from glfusion_amd.models.layers import conv_bn_act
    n, h, w, ho, wo, k, _, stride, pad, dil = geo
    relu, want_rect = CASES[name][9], CASES[name][11]
    cout, cin = conv.weight.shape[0], conv.weight.shape[1]
    truth = _truth64(x, conv, bn, stride, pad, dil, relu, res)
    emu = _emulation(x, conv, bn, stride, pad, dil, relu, res)
    plain, mask, rect, pho, pwo = _plan(x, conv, bn, stride, pad, dil)
    assert rect == want_rect and (pho, pwo) == (ho, wo)
    wf, shift = _fold_direct(conv, bn)
    y = _nan_filled(n, ho, wo, cout)
    p = _gparams(n * ho * wo, cout, cin, cout, None if plain else geo, mask, rect)
    _epilogue_call(x, wf, y, p, shift, res, cout if res is not None else 0, relu)
    assert bool(torch.isfinite(y.float()).all())
    with ops.precision_scope("bf16"), torch.no_grad():
        assert not ops.fold_bn_s16()
        y_unf = conv_bn_act(x, conv, bn, relu=relu, residual=res)
        torch.cuda.synchronize()
    return _rel(y, truth), _rel(emu, truth), _rel(y_unf, truth)


# ------------------------------------------------------------------------------------------------ 1. folded conv against float64
@pytest.mark.parametrize("name", list(CASES))
def test_folded_conv_vs_float64(name):
    """glf_s16_fold_bn + glf_s16_gemm_nt_epilogue against the float64 conv -> eval BatchNorm -> add -> ReLU.  Gate: relative L2 error
    <= 1.5 x the error of the emulation of the same roundings (bf16 W' from the double product, one bf16 rounding of the result); every
    element finite.  The same layer through the unfolded bf16 conv_bn_act is printed as a record."""
    err_k, err_e, err_u = _folded_vs_float64(name, *_case(name))
    print(f"{name}: relative L2 vs float64: folded kernel {err_k:.3e}, emulation {err_e:.3e}, unfolded bf16 pair {err_u:.3e}")
    assert err_k <= 1.5 * err_e, (err_k, err_e)


# ------------------------------------------------------------------------------------------------ 2. mean-dominated channel
def test_mean_dominated_channel():
    """Case a with a constant added to the input so that every conv channel's mean is about 40 x its spread (the weights of a channel
    sum to one, the constant is 40), running_mean set to that mean.  Unfolded, the conv output is rounded to bf16 with most mantissa
    bits spent on the mean; folded, the mean cancels against the shift in fp32.  Same gate; the two errors are printed side by side."""
    name = "a_1x1_res_relu"
    conv, bn, x, res, geo = _case(name)
    with torch.no_grad():
        w = conv.weight
        w.add_((1.0 - w.sum(dim=(1, 2, 3), keepdim=True)) / w[0].numel())
    x = (x.float() + 40.0).to(BF)
    y64 = _conv64(x.double(), conv.weight.detach().double(), 1, 0, 1).reshape(-1, conv.weight.shape[0])
    mean, spread = y64.mean(0), y64.std(0)
    ratio = float((mean.abs() / spread).median())
    assert 20.0 <= ratio <= 80.0, ratio
    with torch.no_grad():
        bn.running_mean.copy_(mean.float())
    err_k, err_e, err_u = _folded_vs_float64(name, conv, bn, x, res, geo)
    print(f"mean-dominated ({ratio:.1f} x spread): relative L2 vs float64: folded kernel {err_k:.3e}, emulation {err_e:.3e}, "
          f"unfolded bf16 pair {err_u:.3e}")
    assert err_k <= 1.5 * err_e, (err_k, err_e)


# ------------------------------------------------------------------------------------------------ 3. the fold kernel
@pytest.mark.parametrize("bias", [False, True])
def test_fold_kernel_bit_exact(bias):
    """W' is EXACTLY the bf16 nearest-even rounding of the double product W * s (bit patterns; no allowance), the shift matches the
    float64 formula to fp32 rounding.  With and without a conv bias."""
    from glfusion_amd import ops
    conv, bn = _conv_bn(40, 20, 3, 1, 1, 1, seed=3, bias=bias)
    if bias:
        with torch.no_grad():
            conv.bias.copy_(torch.randn(20, generator=torch.Generator().manual_seed(4)))
    wf, shift = _fold_direct(conv, bn)
    torch.cuda.synchronize()
    s = _scale64(bn)
    want_w = _bf16_rne(ops.tap_major(conv.weight).double() * s[None, :, None])
    diff = int((_bits(wf) != _bits(want_w)).sum())
    assert diff == 0, f"{diff} of {wf.numel()} folded weights differ from the single nearest-even rounding"
    b = conv.bias.detach().double() if bias else 0.0
    want_b = bn.bias.detach().double() + (b - bn.running_mean.double()) * s
    assert bool(((shift.double() - want_b).abs() <= 0.51 * 2.0 ** -23 * want_b.abs() + 1e-30).all())


def test_fold_kernel_rounds_once_where_two_roundings_differ():
    """A product W * s just above a bf16 tie, by less than half an fp32 ulp: W = 1 + 2^-8 (the tie between 1 and 1 + 2^-7),
    s = 1 / sqrt(1 - 2^-24) ~ 1 + 2^-25.  An fp32 W' would land ON the tie and round down to even (two roundings); the single
    rounding of the double product goes up.  The kernel must round up."""
    from glfusion_amd.models.layers import BatchNorm2d, Conv2d
    conv, bn = Conv2d(8, 1, 1, bias=False).to(DEV), BatchNorm2d(1, eps=0.0).to(DEV).eval()
    with torch.no_grad():
        conv.weight.fill_(1.0 + 2.0 ** -8)
        bn.weight.fill_(1.0)
        bn.running_var.fill_(1.0 - 2.0 ** -24)
    wf, _ = _fold_direct(conv, bn)
    torch.cuda.synchronize()
    prod = conv.weight.detach().double() * _scale64(bn)
    assert float(prod[0, 0, 0, 0]) > 1.0 + 2.0 ** -8
    assert float(prod.float().to(BF)[0, 0, 0, 0]) == 1.0                          # two roundings: down to even
    assert bool((wf.float() == 1.0 + 2.0 ** -7).all()), wf.float().flatten().tolist()


# ------------------------------------------------------------------------------------------------ 4. write discipline
@pytest.mark.parametrize("N,ldc,col0,with_res", [(128, 320, 64, True), (72, 137, 0, False)])
def test_epilogue_write_discipline(N, ldc, col0, with_res):
    """Output = a column slice of a wider buffer (ldc = 320, columns 64 .. 191: the 16-byte store path; N = 72, ldc = 137: the
    one-element path), slice, padding and extra rows pre-filled with a NaN pattern: the slice comes out wholly finite and right, every
    element outside it keeps its bits."""
    M, K, extra = 392, 64, 3
    g = torch.Generator().manual_seed(11)
    A, B = torch.randn(M, K, generator=g).to(DEV).to(BF), (torch.randn(N, K, generator=g) / 8).to(DEV).to(BF)
    shift = torch.randn(N, generator=g).to(DEV)
    res = torch.randn(M, N + 8, generator=g).to(DEV).to(BF) if with_res else None
    buf = _nan_filled(M + extra, ldc)
    _epilogue_call(A, B, buf[:, col0:], _gparams(M, N, K, ldc), shift, res, N + 8 if with_res else 0, relu=1)
    inside = torch.zeros(M + extra, ldc, dtype=torch.bool, device=DEV)
    inside[:M, col0:col0 + N] = True
    assert bool((_bits(buf)[~inside] == NAN_BITS).all())
    out = buf[:M, col0:col0 + N].float()
    assert bool(torch.isfinite(out).all())
    want = A.double() @ B.double().t() + shift.double() + (res[:, :N].double() if with_res else 0.0)
    assert _rel(out, torch.relu(want)) <= 2.0 ** -8                                # one bf16 rounding of every element: <= 2^-9 each


# ------------------------------------------------------------------------------------------------ 5. epilogue off = the plain kernel
@pytest.mark.parametrize("name", ["a_1x1_res_relu", "b_3x3_s2_relu"])
def test_epilogue_off_equals_plain_kernel(name):
    """No residual, relu = 0, shift = b: bitwise the bf16 result of glf_s16_gemm_nt with bias = b."""
    from glfusion_amd import ops
    from glfusion_amd._lib import check, lib
    conv, bn, x, _, geo = _case(name)
    n, h, w, ho, wo, k, _, stride, pad, dil = geo
    cout, cin = conv.weight.shape[0], conv.weight.shape[1]
    plain, mask, rect, _, _ = _plan(x, conv, bn, stride, pad, dil)
    wf, shift = _fold_direct(conv, bn)
    p = _gparams(n * ho * wo, cout, cin, cout, None if plain else geo, mask, rect)
    y_epi, y_plain = _nan_filled(n, ho, wo, cout), _nan_filled(n, ho, wo, cout)
    _epilogue_call(x, wf, y_epi, p, shift)
    check(lib.glf_s16_gemm_nt(ops._p(x), ops._p(wf), ops._p(shift), ops._p(y_plain), C.byref(p), ops._stream()), "s16_gemm_nt")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y_plain.float()).all())
    assert torch.equal(_bits(y_epi), _bits(y_plain))


# ------------------------------------------------------------------------------------------------ 6. staleness
def test_staleness_of_folded_images():
    """Each of the six sources (conv weight, conv bias, gamma, beta, running_mean, running_var): an in-place write re-folds exactly
    once, a replaced tensor re-folds exactly once, an untouched second call does not re-fold; ops.stats_moved() re-folds."""
    from glfusion_amd import ops
    from glfusion_amd.models.layers import conv_bn_act
    from torch import nn
    ops.set_precision("bf16")
    ops.set_fold_bn_s16(True)
    conv, bn = _conv_bn(64, 64, 3, 1, 1, 1, seed=5, bias=True)
    x = torch.randn(2, 10, 10, 64, generator=torch.Generator().manual_seed(1)).to(DEV).to(BF)

    def run(expect):
        before = ops.FOLD_COUNT[0]
        with torch.no_grad():
            y = conv_bn_act(x, conv, bn, relu=True).clone()
        torch.cuda.synchronize()
        assert ops.FOLD_COUNT[0] - before == expect, (ops.FOLD_COUNT[0] - before, expect)
        return y

    y = run(1)
    assert torch.equal(run(0), y)
    sources = [(conv, "weight"), (conv, "bias"), (bn, "weight"), (bn, "bias"), (bn, "running_mean"), (bn, "running_var")]
    for mod, attr in sources:
        with torch.no_grad():
            getattr(mod, attr).mul_(1.25)                                         # in place: the version counter moves
        y1 = run(1)
        assert not torch.equal(y1, y), attr
        assert torch.equal(run(0), y1), attr
        new = getattr(mod, attr).detach().clone() * 0.8                           # replaced: another tensor, version 0
        setattr(mod, attr, nn.Parameter(new) if isinstance(getattr(mod, attr), nn.Parameter) else new)
        y = run(1)
        assert not torch.equal(y, y1), attr
        assert torch.equal(run(0), y), attr
    ops.stats_moved()
    assert torch.equal(run(1), y)
    ops.stats_moved(bn)
    assert torch.equal(run(1), y)
    assert torch.equal(run(0), y)


# ------------------------------------------------------------------------------------------------ 7. off the path
def _bottleneck(inplanes, planes, stride, seed):
    from glfusion_amd.models.layers import BatchNorm2d, Conv2d
    from glfusion_amd.models.resnet import Bottleneck
    from torch import nn
    torch.manual_seed(seed)
    down = nn.Sequential(Conv2d(inplanes, planes * 4, 1, stride=stride, bias=False), BatchNorm2d(planes * 4))
    blk = Bottleneck(inplanes, planes, stride, down)
    for i, m in enumerate(blk.modules()):
        if isinstance(m, BatchNorm2d):
            _bn_fill(m, seed + 10 + i, 0.3)
    return blk


def _run16(blk, x_nhwc16):
    with torch.no_grad():
        y = blk.forward_nhwc(x_nhwc16).clone()
    torch.cuda.synchronize()
    return y


def _x16(seed, n=2, c=64, hw=14):
    return torch.randn(n, hw, hw, c, generator=torch.Generator().manual_seed(seed)).to(DEV).to(BF)


@pytest.mark.parametrize("what", ["train", "grad", "f16x3"])
def test_no_behaviour_change_off_the_path(what):
    """set_fold_bn_s16(True) changes nothing in train(), with grad enabled, or under 'f16x3': bitwise the switch-off output, and no fold."""
    from glfusion_amd import ops
    ops.set_precision("f16x3" if what == "f16x3" else "bf16")
    x = _x16(2)
    outs = []
    for flag in (False, True):
        ops.set_fold_bn_s16(flag)
        blk = _bottleneck(64, 64, 1, seed=6).to(DEV)
        blk = blk.train() if what == "train" else blk.eval()
        before = ops.FOLD_COUNT[0]
        if what == "grad":
            y = blk.forward_nhwc(x).clone()
        elif what == "f16x3":
            with torch.no_grad():
                y = blk.forward_nhwc(x.float()).clone()
        else:
            y = _run16(blk, x)
        torch.cuda.synchronize()
        assert ops.FOLD_COUNT[0] == before
        outs.append(y.detach())
    assert torch.equal(outs[0], outs[1])


def test_switches_are_independent_and_nothing_is_clobbered():
    """Under 'bf16', set_fold_bn(True) alone folds nothing; after a folded run, switching off reproduces the earlier unfolded output
    bitwise (no shared weight image was clobbered)."""
    from glfusion_amd import ops
    ops.set_precision("bf16")
    blk = _bottleneck(64, 64, 1, seed=8).to(DEV).eval()
    x = _x16(3)
    y_before = _run16(blk, x)
    ops.set_fold_bn(True)
    before = ops.FOLD_COUNT[0]
    assert torch.equal(_run16(blk, x), y_before)
    assert ops.FOLD_COUNT[0] == before
    ops.set_fold_bn(False)
    ops.set_fold_bn_s16(True)
    y_folded = _run16(blk, x)
    assert ops.FOLD_COUNT[0] == before + 4                                        # conv1, conv2, conv3, downsample
    print(f"folded vs unfolded bf16 block: relative L2 {_rel(y_folded, y_before.double()):.3e}")
    ops.set_fold_bn_s16(False)
    assert torch.equal(_run16(blk, x), y_before)


def test_residual_shape_mismatch_raises():
    from glfusion_amd import ops, ops16
    ops.set_precision("bf16")
    ops.set_fold_bn_s16(True)
    conv, bn = _conv_bn(64, 64, 1, 1, 0, 1, seed=2)
    x = _x16(5)
    with torch.no_grad():
        plan = ops16.fold_plan16(x, conv.weight, bn, 1, 0, 1)
        assert plan is not None
        with pytest.raises(RuntimeError, match="residual shape"):
            ops16.conv_bn_folded16(x, conv.weight, None, bn, 1, 0, 1, True, residual=x[:, :7].contiguous(), plan=plan)


# ------------------------------------------------------------------------------------------------ 8. the model against the reference's fixture
def test_model_vs_golden_folded(golden_dir):
    """Global_and_Local on tests/golden/e2e_eval_c2.npz under 'bf16' with the switch on: the gates of
    tests/test_gpu_s16.py::test_s16_e2e_eval_vs_golden (logits within 6e-2 of the largest logit, Dice within 2e-3); the backbone takes
    the path (>= 50 folds).  Folded-vs-reference is printed beside unfolded-vs-reference."""
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    g = np.load(os.path.join(golden_dir, "e2e_eval_c2.npz"))
    views, n = ["1", "3", "4"], 2
    ops.set_precision("bf16")
    model = Global_and_Local(views)
    orc.closed_form_fill(model, salt=1)
    model = model.to(DEV).eval()
    imgs = {v: t.to(DEV) for v, t in orc.closed_form_images(views, n).items()}
    tgts = orc.closed_form_targets(views, n)
    with torch.no_grad():
        unf = model(imgs)
        ops.set_fold_bn_s16(True)
        before = ops.FOLD_COUNT[0]
        mask, mask_bb, f4g, f4l = model(imgs)
    torch.cuda.synchronize()
    assert ops.FOLD_COUNT[0] - before >= 50, "the folded path was not taken by the backbone"
    for v in views:
        assert mask[v].dtype == torch.float32 and f4g[v].dtype == BF
        for got, got_u, key in ((mask[v], unf[0][v], f"mask:{v}"), (mask_bb[v], unf[1][v], f"mask_bb:{v}")):
            ref = torch.from_numpy(g[key])
            err = float((got.cpu() - ref).abs().max()) / float(ref.abs().max())
            err_u = float((got_u.cpu() - ref).abs().max()) / float(ref.abs().max())
            print(f"{key}: max |logit - reference| / max |reference|: folded {err:.3e}, unfolded {err_u:.3e}")
            assert err <= 6e-2, (key, err)
        dice = ops.overlap_metrics_from_counts(ops.overlap_counts(mask[v], tgts[v].to(DEV)))
        dice_u = ops.overlap_metrics_from_counts(ops.overlap_counts(unf[0][v], tgts[v].to(DEV)))
        print(f"view {v}: Dice folded {dice[1]:.5f}, unfolded {dice_u[1]:.5f}, reference {float(g[f'dice:{v}'][1]):.5f}")
        assert abs(dice[1] - float(g[f"dice:{v}"][1])) <= 2e-3, (v, dice[1], float(g[f"dice:{v}"][1]))


# ------------------------------------------------------------------------------------------------ 9. graph capture
def test_graph_capture_of_a_folded_forward():
    """A folded eval forward of Bottleneck(256 -> 512, stride 2) under 'bf16', captured in torch.cuda.graph after a side-stream warm-up,
    replays bitwise equal to the eager result (no host synchronisation, no allocation outside torch's allocator).  The folded images are
    not part of the graph: after running_mean changed, a replay still computes with the old images until an eager forward re-folds them
    (in place: the graph reads the same buffers), and then equals the new eager result."""
    from glfusion_amd import ops
    ops.set_precision("bf16")
    ops.set_fold_bn_s16(True)
    blk = _bottleneck(256, 128, 2, seed=9).to(DEV).eval()
    x = _x16(4, c=256, hw=15)
    eager = _run16(blk, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            blk.forward_nhwc(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.reset_capture_pools()
    graph = torch.cuda.CUDAGraph()
    count = ops.FOLD_COUNT[0]
    with torch.no_grad(), torch.cuda.graph(graph):
        static = blk.forward_nhwc(x)
    assert ops.FOLD_COUNT[0] == count                                            # the capture re-folded nothing
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)
    with torch.no_grad():
        blk.bn3.running_mean.add_(0.5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager)                                            # nothing re-folded yet
    eager2 = _run16(blk, x)                                                      # the eager forward notices and re-folds in place
    assert ops.FOLD_COUNT[0] == count + 1 and not torch.equal(eager2, eager)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static, eager2)
    del graph
    ops.reset_capture_pools()


# ------------------------------------------------------------------------------------------------ 10. Trainer
def test_trainer_switch():
    """config['train']['fold_bn_s16'] = True with precision 'bf16': eval() folds, restores the switch afterwards, and returns Dice
    within 2e-3 of the switch-off run on the same synthetic patients."""
    from glfusion_amd import ops
    from glfusion_amd.data import SyntheticPatients
    from glfusion_amd.engine import Trainer
    views = ["1", "4"]
    results = {}
    for flag in (False, True):
        cfg = {"train": {"batch_size": 1, "num_epochs": 1, "clip_length": 3, "view_num": views, "test_view": views, "save_dir": "/tmp/glf_eval",
                         "iters_per_epoch": 1, "global_rank": 0, "precision": "bf16", "fold_bn_s16": flag},
               "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}}
        t = Trainer(cfg)
        ref = orc.Global_and_Local(views)
        orc.closed_form_fill(ref, salt=9)
        t.model.load_state_dict(ref.state_dict(), strict=True)
        patients = SyntheticPatients(views, 2, clip_length=3, h0=150, w0=170, device=DEV, seed=5)
        before = ops.FOLD_COUNT[0]
        assert not ops.fold_bn_s16()
        results[flag] = t.eval(patients=patients)
        assert not ops.fold_bn_s16()                                             # restored
        assert (ops.FOLD_COUNT[0] > before) == flag
    for v in views:
        print(f"view {v}: metrics folded {np.asarray(results[True][v])}, unfolded {np.asarray(results[False][v])}")
        assert np.allclose(results[True][v], results[False][v], atol=2e-3, rtol=0), (v, results[True][v], results[False][v])
