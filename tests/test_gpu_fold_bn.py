"""GPU: opt-in folded-BatchNorm inference on the split-fp16 kernels (ops.set_fold_bn; glf_fold_bn, glf_gemm_nt_epilogue,
glf_conv2d_fwd_folded): kernel-level accuracy against float64 on the device, write discipline, staleness of the folded images, no change
of behaviour off the path, the full model against the reference's golden outputs, and hipGraph capture."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import glfusion_ref as orc   # the checker (tests only)

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _switch_off_afterwards():
    from glfusion_amd import ops
    yield
    ops.set_fold_bn(False)
    ops.set_precision("f32")


def _bn_fill(bn, seed, spread):
    """BatchNorm parameters that make the fold matter: gamma in [0.5, 1.5] with a few negatives, running_var spread over 1e-2 ... 1e2,
    running_mean of the order of the conv output's spread."""
    g = torch.Generator().manual_seed(seed)
    c = bn.num_features
    gamma = 0.5 + torch.rand(c, generator=g)
    gamma[::7] *= -1.0
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(torch.randn(c, generator=g))
        bn.running_mean.copy_(torch.randn(c, generator=g) * spread)
        bn.running_var.copy_(10.0 ** (torch.rand(c, generator=g) * 4.0 - 2.0))


def _conv_bn(cin, cout, k, stride, pad, dil, seed):
    from glfusion_amd.models.layers import BatchNorm2d, Conv2d
    torch.manual_seed(seed)
    conv = Conv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(cout, cin, k, k) / (cin * k * k) ** 0.5)      # zero mean, conv output spread ~ 1
    bn = BatchNorm2d(cout)
    _bn_fill(bn, seed + 1, 1.0)
    return conv.to(DEV), bn.to(DEV).eval()


def _truth64(x_nhwc, conv, bn, stride, pad, dil, relu, residual):
    """float64 on the device: conv (im2col + matmul) -> eval BatchNorm -> (+ residual) -> (ReLU), from the UNFOLDED parameters."""
    x = x_nhwc.double().permute(0, 3, 1, 2)
    n = x.shape[0]
    cout, cin, k, _ = conv.weight.shape
    ho = (x.shape[2] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (x.shape[3] + 2 * pad - dil * (k - 1) - 1) // stride + 1
    cols = F.unfold(x, k, dilation=dil, padding=pad, stride=stride)                  # [n, cin*k*k, ho*wo]
    y = torch.matmul(conv.weight.double().reshape(cout, -1), cols)                   # [n, cout, ho*wo]
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    y = (y - bn.running_mean.double()[None, :, None]) * s[None, :, None] + bn.bias.double()[None, :, None]
    y = y.reshape(n, cout, ho, wo).permute(0, 2, 3, 1)
    if residual is not None:
        y = y + residual.double()
    return torch.relu(y) if relu else y


def _rel(a, b):
    a, b = a.detach().double(), b.detach()
    return float((a - b).norm() / b.norm())


def _fold_direct(conv, bn):
    """(tap-major folded weights, shift) through glf_fold_bn itself."""
    from glfusion_amd import ops
    from glfusion_amd._lib import check, lib
    cout, cin, k, _ = conv.weight.shape
    wt = ops.tap_major(conv.weight)
    wf = torch.empty(k * k, cout, cin, device=DEV)
    shift = torch.empty(cout, device=DEV)
    check(lib.glf_fold_bn(ops._p(wt), None, ops._p(bn.weight.detach()), ops._p(bn.bias.detach()), ops._p(bn.running_mean), ops._p(bn.running_var),
                          float(bn.eps), ops._p(wf), ops._p(shift), k * k, cout, cin, ops._stream()), "fold_bn")
    return wf, shift


CASES = {
    # name: (n, h, w, cin, cout, k, stride, pad, dil, relu, residual, plan rect)
    "a_1x1_res_relu": (2, 14, 14, 64, 256, 1, 1, 0, 1, True, True, 0),          # M = 392: ragged row tile, 64-wide K
    "b_3x3_s2_relu": (2, 17, 17, 128, 128, 3, 2, 1, 1, True, False, 0),         # gather, stride 2, odd map
    "c_3x3_dil2_identity": (2, 14, 14, 256, 256, 3, 1, 2, 2, False, False, 0),
    "d_3x3_dil12_region_relu": (1, 28, 28, 512, 256, 3, 1, 12, 12, True, False, 2),
    "e_1x1_shift_only": (2, 9, 11, 256, 64, 1, 1, 0, 1, False, False, 0),
}


@pytest.mark.parametrize("name", list(CASES))
def test_folded_conv_vs_float64(name):
    """glf_conv2d_fwd_folded against the float64 conv -> eval BatchNorm -> add -> ReLU.  The project gates plain split-fp16 contractions
    at 2e-6 relative L2 against float64 and the fold adds one fp32 rounding of W * scale, so: err_folded <= max(2 * err_unfolded, 2e-6),
    err_unfolded being the same layer through today's conv + batch_norm_act eval path, measured here."""
    from glfusion_amd import ops
    from glfusion_amd._lib import ConvParams, ConvPlan, check, lib
    from glfusion_amd.models.layers import conv_bn_act
    n, h, w, cin, cout, k, stride, pad, dil, relu, has_res, want_rect = CASES[name]
    conv, bn = _conv_bn(cin, cout, k, stride, pad, dil, seed=len(name))
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n, h, w, cin, generator=g).to(DEV)
    ho = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dil * (k - 1) - 1) // stride + 1
    res = torch.randn(n, ho, wo, cout, generator=g).to(DEV) if has_res else None
    truth = _truth64(x, conv, bn, stride, pad, dil, relu, res)
    with ops.precision_scope("f16x3"), torch.no_grad():
        assert not ops.fold_bn()
        y_unf = conv_bn_act(x, conv, bn, relu=relu, residual=res)
        wf, shift = _fold_direct(conv, bn)
        p = ConvParams()
        p.n, p.h, p.w, p.cin, p.cout, p.kh, p.kw, p.stride, p.pad, p.dil, p.precision = n, h, w, cin, cout, k, k, stride, pad, dil, 3
        pl = ConvPlan()
        check(lib.glf_conv2d_plan(C.byref(p), 3, C.byref(pl)), "plan")
        assert pl.rect == want_rect and (pl.ho, pl.wo) == (ho, wo)
        amax_out = torch.zeros(1, device=DEV)
        p.amax_out = ops._p(amax_out)
        y = torch.full((n, ho, wo, cout), float("nan"), device=DEV)
        check(lib.glf_conv2d_fwd_folded(ops._p(x), ops._p(wf), ops._p(shift), ops._p(res), cout, int(relu), ops._p(y), C.byref(p), ops._stream()), "folded")
        torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all())
    err_f, err_u = _rel(y, truth), _rel(y_unf, truth)
    print(f"{name}: relative L2 vs float64: folded {err_f:.3e}, unfolded {err_u:.3e}")
    assert err_f <= max(2.0 * err_u, 2e-6), (err_f, err_u)
    assert float(amax_out) == float(y.abs().max())                                # the maximum of the value actually stored


def test_fold_bn_kernel_vs_float64():
    """glf_fold_bn: folded weights and shift (with a conv bias) against the float64 formulas, to fp32 rounding."""
    from glfusion_amd import ops
    from glfusion_amd._lib import check, lib
    conv, bn = _conv_bn(36, 20, 3, 1, 1, 1, seed=3)
    bias = torch.randn(20, device=DEV)
    wt = ops.tap_major(conv.weight)
    wf, shift = torch.empty_like(wt), torch.empty(20, device=DEV)
    check(lib.glf_fold_bn(ops._p(wt), ops._p(bias), ops._p(bn.weight.detach()), ops._p(bn.bias.detach()), ops._p(bn.running_mean), ops._p(bn.running_var),
                          float(bn.eps), ops._p(wf), ops._p(shift), 9, 20, 36, ops._stream()), "fold_bn")
    s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
    want_w = wt.double() * s[None, :, None]
    want_b = bn.bias.double() + (bias.double() - bn.running_mean.double()) * s
    eps32 = 2.0 ** -23                                                            # one rounding of the scale, one of the product
    assert bool(((wf.double() - want_w).abs() <= 1.01 * eps32 * want_w.abs()).all())
    assert bool(((shift.double() - want_b).abs() <= 0.51 * eps32 * want_b.abs() + 1e-30).all())


@pytest.mark.parametrize("ldc", [144, 137])
def test_epilogue_write_discipline(ldc):
    """glf_gemm_nt_epilogue into a buffer with a padded row stride (144: the 16-byte store path, 137: the one-dword path), NaN sentinels
    outside the written slice and extra rows: the sentinels survive, everything inside is finite, two runs are bitwise equal."""
    from glfusion_amd import ops
    from glfusion_amd._lib import GemmEpilogue, GemmParams, check, lib
    M, N, K, extra = 300, 136, 64, 5
    g = torch.Generator().manual_seed(11)
    A, B = torch.randn(M, K, generator=g).to(DEV), torch.randn(N, K, generator=g).to(DEV)
    shift = torch.randn(N, generator=g).to(DEV)
    ld_res = 140
    res = torch.randn(M, ld_res, generator=g).to(DEV)
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, K, K, K, ldc
    p.taps, p.tap_mask, p.gather = 1, 1, 0
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = (1, 1, 1, 1, 1, 1, 1, 1, 0, 1)
    p.batch, p.alpha, p.split, p.precision = 1, 1.0, 1, 3
    e = GemmEpilogue()
    e.shift, e.residual, e.ld_res, e.relu = shift.data_ptr(), res.data_ptr(), ld_res, 1
    outs = []
    for _ in range(2):
        buf = torch.full((M + extra, ldc), float("nan"), device=DEV)
        check(lib.glf_gemm_nt_epilogue(ops._p(A), ops._p(B), ops._p(buf), C.byref(p), C.byref(e), ops._stream()), "gemm_nt_epilogue")
        torch.cuda.synchronize()
        outs.append(buf)
    buf = outs[0]
    assert bool(torch.isfinite(buf[:M, :N]).all())
    assert bool(torch.isnan(buf[:M, N:]).all()) and bool(torch.isnan(buf[M:]).all())
    assert torch.equal(outs[0][:M, :N], outs[1][:M, :N])
    want = torch.relu(A.double() @ B.double().t() + shift.double() + res[:, :N].double())
    assert _rel(buf[:M, :N], want) <= 2e-6


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


def _run(blk, x):
    with torch.no_grad():
        y = blk(x).contiguous().clone()
    torch.cuda.synchronize()
    return y


def test_staleness_of_folded_images():
    """Folded images are rebuilt when a source changes (a weight in place, running statistics in place, load_state_dict) -- the output
    then equals a freshly constructed module's folded output bitwise -- and never otherwise: five unchanged forwards launch no glf_fold_bn."""
    from glfusion_amd import ops
    ops.set_precision("f16x3")
    ops.set_fold_bn(True)
    blk = _bottleneck(64, 64, 1, seed=5).to(DEV).eval()
    x = torch.randn(2, 64, 14, 14, generator=torch.Generator().manual_seed(1)).to(DEV)

    def fresh_output():
        twin = _bottleneck(64, 64, 1, seed=99)
        twin.load_state_dict({k: v.clone() for k, v in blk.state_dict().items()})
        return _run(twin.to(DEV).eval(), x)

    before = ops.FOLD_COUNT[0]
    y0 = _run(blk, x)
    assert ops.FOLD_COUNT[0] == before + 4                                       # conv1, conv2, conv3, downsample
    ops.set_fold_bn(False)
    y_unf = _run(blk, x)
    ops.set_fold_bn(True)
    assert float((y0 - y_unf).abs().max()) <= 1e-4 * float(y_unf.abs().max())    # the folded block computes the block
    assert torch.equal(y0, fresh_output())
    with torch.no_grad():
        blk.conv2.weight.mul_(1.25)
    y1 = _run(blk, x)
    assert not torch.equal(y1, y0) and torch.equal(y1, fresh_output())
    with torch.no_grad():
        blk.bn3.running_var.mul_(0.5)
    y2 = _run(blk, x)
    assert not torch.equal(y2, y1) and torch.equal(y2, fresh_output())
    sd = {k: (v * 1.01 if v.is_floating_point() else v.clone()) for k, v in blk.state_dict().items()}
    blk.load_state_dict(sd)
    y3 = _run(blk, x)
    assert not torch.equal(y3, y2) and torch.equal(y3, fresh_output())
    count = ops.FOLD_COUNT[0]
    for _ in range(5):
        assert torch.equal(_run(blk, x), y3)
    assert ops.FOLD_COUNT[0] == count
    # a train-mode forward moves the running statistics through raw kernel writes: the images notice
    blk.train()
    with torch.no_grad():
        blk(x)
    blk.eval()
    y4 = _run(blk, x)
    assert ops.FOLD_COUNT[0] == count + 4
    assert torch.equal(y4, fresh_output())


@pytest.mark.parametrize("what", ["train", "grad", "f32", "bf16"])
def test_no_behaviour_change_off_the_path(what):
    """Fold on changes nothing in train(), with grad enabled, or under the 'f32' / 'bf16' precisions: bitwise the fold-off output."""
    from glfusion_amd import ops
    ops.set_precision({"f32": "f32", "bf16": "bf16"}.get(what, "f16x3"))
    x = torch.randn(2, 64, 14, 14, generator=torch.Generator().manual_seed(2)).to(DEV)
    outs = []
    for flag in (False, True):
        ops.set_fold_bn(flag)
        blk = _bottleneck(64, 64, 1, seed=6).to(DEV)
        blk = blk.train() if what == "train" else blk.eval()
        before = ops.FOLD_COUNT[0]
        if what == "grad":
            y = blk(x).contiguous().clone()
        elif what == "bf16":
            from glfusion_amd import ops16
            with torch.no_grad():
                y = blk.forward_nhwc(ops16.to_bf16(ops.to_nhwc(x))).clone()
        else:
            y = _run(blk, x)
        torch.cuda.synchronize()
        assert ops.FOLD_COUNT[0] == before
        outs.append(y.detach())
    assert torch.equal(outs[0], outs[1])


def test_fold_off_is_untouched_by_the_folded_path():
    """With fold off the f16x3 eval output of the block is bitwise the same before and after the folded path ran in the process: no
    shared weight image was clobbered."""
    from glfusion_amd import ops
    ops.set_precision("f16x3")
    blk = _bottleneck(64, 64, 1, seed=8).to(DEV).eval()
    x = torch.randn(2, 64, 14, 14, generator=torch.Generator().manual_seed(3)).to(DEV)
    y_before = _run(blk, x)
    ops.set_fold_bn(True)
    before = ops.FOLD_COUNT[0]
    _run(blk, x)
    assert ops.FOLD_COUNT[0] > before
    ops.set_fold_bn(False)
    assert torch.equal(_run(blk, x), y_before)


def test_model_vs_golden_folded(golden_dir):
    """Global_and_Local from tests/golden/e2e_eval_c1.npz under f16x3 with fold on: the gates of test_gpu_model.py::test_e2e_eval_vs_golden
    (logits within 1e-4 of the reference's outputs, Dice within 1e-4)."""
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local
    tol = 1e-4
    views, n = ["1"], 8
    g = np.load(os.path.join(golden_dir, "e2e_eval_c1.npz"))
    ops.set_precision("f16x3")
    model = Global_and_Local(views)
    orc.closed_form_fill(model, salt=1)
    model = model.to(DEV).eval()
    imgs = {v: t.to(DEV) for v, t in orc.closed_form_images(views, n).items()}
    tgts = orc.closed_form_targets(views, n)
    with torch.no_grad():
        unf = model(imgs)
        ops.set_fold_bn(True)
        before = ops.FOLD_COUNT[0]
        mask, mask_bb, fg, fl = model(imgs)
    torch.cuda.synchronize()
    assert ops.FOLD_COUNT[0] - before >= 50, "the folded path was not taken by the backbone"

    for v in views:
        d_ref = float((mask[v].cpu() - torch.from_numpy(g[f"mask:{v}"])).abs().max())
        d_unf = float((mask[v] - unf[0][v]).abs().max())
        print(f"view {v}: max |logit - reference| {d_ref:.3e} (reference max |logit| {float(np.abs(g[f'mask:{v}']).max()):.3e}); "
              f"folded vs unfolded {d_unf:.3e}")
        assert tuple(mask[v].shape) == (n, 5, 112, 112)
        assert _golden_close(mask[v], g[f"mask:{v}"], tol), v
        assert _golden_close(mask_bb[v], g[f"mask_bb:{v}"], tol), v
        ref = torch.from_numpy(g[f"mask:{v}"])
        differ = orc.binarize(mask[v].cpu()) != orc.binarize(ref)
        assert bool((ref.abs()[differ] < tol).all())
        dice = ops.overlap_metrics_from_counts(ops.overlap_counts(mask[v], tgts[v].to(DEV)))
        assert np.allclose(dice, g[f"dice:{v}"], atol=tol, rtol=0), (dice, g[f"dice:{v}"])


def _golden_close(a, b, tol):
    """The gate of tests/test_gpu_model.py (close): |a - b| <= tol + tol * |b| element by element."""
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    return bool(((a - b).abs() <= tol + tol * b.abs()).all())


def test_graph_capture_of_a_folded_forward():
    """A folded eval forward of Bottleneck(256 -> 512, stride 2), captured in torch.cuda.graph after a side-stream warm-up, replays bitwise
    equal to the eager result: no host synchronisation, no allocation outside torch's allocator."""
    from glfusion_amd import ops
    ops.set_precision("f16x3")
    ops.set_fold_bn(True)
    blk = _bottleneck(256, 128, 2, seed=9).to(DEV).eval()
    x = torch.randn(2, 256, 15, 15, generator=torch.Generator().manual_seed(4)).to(DEV)
    eager = _run(blk, x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            blk(x)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ops.reset_capture_pools()
    graph = torch.cuda.CUDAGraph()
    count = ops.FOLD_COUNT[0]
    with torch.no_grad(), torch.cuda.graph(graph):
        static = blk(x)
    assert ops.FOLD_COUNT[0] == count                                            # the capture re-folded nothing
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static.contiguous(), eager)
    ops.reset_capture_pools()
