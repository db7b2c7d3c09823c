"""GPU: fused softmax attention under 16-bit storage (csrc/attn_s16.hip: glf_s16_attn_softmax_fwd / _bwd) and the fusion block's
`embedded` mode under precision "bf16" (fusion16.Tpavi16Fn).

Arithmetic contract checked here: S = theta phi^T on bf16 MFMA with fp32 accumulation, row max / sum / rescaling in fp32, P and dS
rounded to bf16 only as MFMA operands, y and the gradients accumulated in fp32 and stored as bf16 once, lse fp32.  The kernel is
gated against float64 on the SAME bf16 inputs, with a bound derived from a torch emulation of exactly those roundings."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import glfusion_ref as orc   # the checker (tests only)

DEV = "cuda"
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _s16_mode():
    from glfusion_amd import ops
    ops.set_precision("bf16")
    yield
    ops.set_precision("f32")


def l2(a, b) -> float:
    a, b = torch.as_tensor(a).detach().double(), torch.as_tensor(b).detach().double().to(torch.as_tensor(a).device)
    return float((a - b).norm()) / max(float(b.norm()), 1e-30)


def _lib():
    from glfusion_amd._lib import lib
    return lib


def _params(frames, L, ci, ld, ldy, ldd=None):
    from glfusion_amd._lib import AttnParams
    p = AttnParams()
    p.frames, p.L, p.ci = frames, L, ci
    p.ldq = p.ldk = p.ldv = ld
    p.ldd = ld if ldd is None else ldd
    p.ldy = p.lddy = ldy
    return p


def _p(t):
    return C.c_void_p(t.data_ptr())


def _check(rc, what):
    assert rc == 0, f"{what}: {_lib().glf_last_error()}"


def _inputs(frames, L, ci, seed, offset=0.0):
    """qkv [rows][3 ci] bf16 with scores of standard deviation ~4; offset != 0: a shared per-row offset of about +-offset on
    every score of a row (phi's column 0 is 1, theta's column 0 the offset)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows = frames * L
    sig = (4.0 / ci ** 0.5) ** 0.5
    qkv = torch.randn(rows, 3 * ci, generator=g) * sig
    qkv[:, 2 * ci:] = torch.randn(rows, ci, generator=g)
    if offset:
        qkv[:, ci] = 1.0
        qkv[:, 0] = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0) * offset
    dy = torch.randn(rows, ci, generator=g)
    return qkv.to(BF).to(DEV), dy.to(BF).to(DEV)


def _reference(qkv, dy, y16, frames, L, ci):
    """float64 truth and the bf16-rounding emulation, per frame: (y, lse, dtheta, dphi, dg) each."""
    q = qkv.double().view(frames, L, 3 * ci)
    th, ph, g = q[..., :ci], q[..., ci:2 * ci], q[..., 2 * ci:]
    dyd = dy.double().view(frames, L, ci)
    S = th @ ph.transpose(1, 2)
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    y = P @ g
    D = (dyd * y).sum(-1, keepdim=True)
    dP = dyd @ g.transpose(1, 2)
    dS = P * (dP - D)
    truth = (y, lse, dS @ ph, dS.transpose(1, 2) @ th, P.transpose(1, 2) @ dyd)
    r = lambda t: t.to(BF).double()                          # noqa: E731
    m = S.max(-1, keepdim=True).values
    E = torch.exp(S - m)
    y_e = r((r(E) @ g) / E.sum(-1, keepdim=True))
    De = (dyd * y16.double().view(frames, L, ci)).sum(-1, keepdim=True)
    dSe = r(P * (dP - De))
    emu = (y_e, lse, r(dSe @ ph), r(dSe.transpose(1, 2) @ th), r(r(P).transpose(1, 2) @ dyd))
    return truth, emu, float(S.abs().max())


def _run(qkv, dy, frames, L, ci):
    rows = frames * L
    y = torch.empty(rows, ci, dtype=BF, device=DEV)
    lse = torch.empty(rows, dtype=torch.float32, device=DEV)
    dqkv = torch.empty(rows, 3 * ci, dtype=BF, device=DEV)
    dsum = torch.empty(rows, dtype=torch.float32, device=DEV)
    p = _params(frames, L, ci, 3 * ci, ci)
    lib = _lib()
    _check(lib.glf_s16_attn_softmax_fwd(_p(qkv), _p(qkv[:, ci:]), _p(qkv[:, 2 * ci:]), _p(y), _p(lse), C.byref(p), None), "fwd")
    _check(lib.glf_s16_attn_softmax_bwd(_p(qkv), _p(qkv[:, ci:]), _p(qkv[:, 2 * ci:]), _p(y), _p(dy), _p(lse), _p(dqkv), _p(dqkv[:, ci:]),
                                        _p(dqkv[:, 2 * ci:]), _p(dsum), C.byref(p), None), "bwd")
    torch.cuda.synchronize()
    return y, lse, dqkv


@pytest.mark.parametrize("frames,L,ci,offset", [(2, 60, 64, 0.0), (3, 360, 128, 0.0), (2, 2352, 1024, 0.0), (2, 200, 128, 296.0)])
def test_s16_attn_kernel_vs_float64(frames, L, ci, offset):
    qkv, dy = _inputs(frames, L, ci, 7 + L + ci, offset)
    y, lse, dqkv = _run(qkv, dy, frames, L, ci)
    truth, emu, smax = _reference(qkv, dy, y, frames, L, ci)
    got = (y.view(frames, L, ci), lse.view(frames, L), dqkv[:, :ci].reshape(frames, L, ci), dqkv[:, ci:2 * ci].reshape(frames, L, ci),
           dqkv[:, 2 * ci:].reshape(frames, L, ci))
    lse_err = float((got[1].double() - truth[1]).abs().max())
    assert lse_err <= 2e-5 * max(1.0, smax), (lse_err, smax)
    msg = []
    for name, k in (("y", 0), ("dtheta", 2), ("dphi", 3), ("dg", 4)):
        assert bool(torch.isfinite(got[k]).all()), name
        e = l2(got[k], truth[k])
        e_emu = l2(emu[k], truth[k])
        msg.append(f"{name} {e:.2e} (emulation {e_emu:.2e})")
        assert e <= max(1.5 * e_emu, 1e-3), (name, e, e_emu)
        assert e <= 2e-2, (name, e)
    print(f"s16 attn {frames}x{L}x{ci} offset {offset}: lse {lse_err:.1e}, " + ", ".join(msg))


def test_s16_attn_write_discipline_and_reproducibility():
    """Every output element written exactly once: NaN sentinels outside the written slices survive, nothing inside them does;
    two backward runs are bitwise equal (no atomics)."""
    frames, L, ci, pad, extra = 2, 100, 128, 64, 7
    rows = frames * L
    qkv, dy = _inputs(frames, L, ci, 21)
    ldy, ldd = ci + pad, 3 * ci + pad
    nan = float("nan")
    ybuf = torch.full((rows + extra, ldy), nan, dtype=BF, device=DEV)
    lse = torch.full((rows + extra,), nan, dtype=torch.float32, device=DEV)
    dsum = torch.full((rows + extra,), nan, dtype=torch.float32, device=DEV)
    p = _params(frames, L, ci, 3 * ci, ldy, ldd)
    lib = _lib()
    dyb = torch.zeros(rows, ldy, dtype=BF, device=DEV)
    dyb[:, :ci] = dy
    _check(lib.glf_s16_attn_softmax_fwd(_p(qkv), _p(qkv[:, ci:]), _p(qkv[:, 2 * ci:]), _p(ybuf), _p(lse), C.byref(p), None), "fwd")
    outs = []
    for _ in range(2):
        d = torch.full((rows + extra, ldd), nan, dtype=BF, device=DEV)
        _check(lib.glf_s16_attn_softmax_bwd(_p(qkv), _p(qkv[:, ci:]), _p(qkv[:, 2 * ci:]), _p(ybuf), _p(dyb), _p(lse), _p(d), _p(d[:, ci:]),
                                            _p(d[:, 2 * ci:]), _p(dsum), C.byref(p), None), "bwd")
        torch.cuda.synchronize()
        outs.append(d)
    assert bool(torch.isfinite(ybuf[:rows, :ci]).all()) and bool(torch.isnan(ybuf[:rows, ci:]).all()) and bool(torch.isnan(ybuf[rows:]).all())
    assert bool(torch.isfinite(lse[:rows]).all()) and bool(torch.isnan(lse[rows:]).all())
    d = outs[0]
    assert bool(torch.isfinite(d[:rows, :3 * ci]).all())
    assert bool(torch.isnan(d[:rows, 3 * ci:]).all()) and bool(torch.isnan(d[rows:]).all())
    assert torch.equal(outs[0][:rows, :3 * ci], outs[1][:rows, :3 * ci])


# ----------------------------------------------------------------------------------------
# the fusion block
# ----------------------------------------------------------------------------------------
def zero_mean_kinkfree_fill(module, seed: int, offset: float = 3.0) -> None:
    """Zero-mean kaiming weights under a seed, BatchNorm betas at +-offset, gamma in [0.9, 1.1] (as in the 16-bit block tests)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv3d, torch.nn.Linear)):
                fan_in = m.weight[0].numel()
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                if m.bias is not None:
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.05)
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


def test_s16_tpavi_embedded_block_vs_oracle():
    from glfusion_amd import ops16
    from glfusion_amd.models.ours import TPAVIModule
    mod = TPAVIModule(in_channels=128, mode="embedded")
    zero_mean_kinkfree_fill(mod, 61)
    ref = orc.TPAVIModule(in_channels=128, mode="embedded")
    ref.load_state_dict(mod.state_dict(), strict=True)
    ref = ref.double().train()
    b0 = {k: b.clone().double() for k, b in mod.named_buffers() if b.dtype.is_floating_point}
    mod = mod.to(DEV).train()
    # input scale 0.5: scores theta . phi of standard deviation ~4 (kaiming projections over 64 channels), the regime of the kernel
    # test above; at scale 1 (~16) the softmax is nearly one-hot and bf16 storage of x alone moves dx by ~5e-2
    x = 0.5 * torch.randn(3, 128, 3, 10, 12, generator=torch.Generator().manual_seed(611))    # [N, C, V, h, w]
    xd = x.to(DEV).requires_grad_(True)
    y = ops16.to_f32(mod.forward_nvhwc(ops16.to_bf16(xd.permute(0, 2, 3, 4, 1).contiguous())))
    xr = x.double().requires_grad_(True)
    yr = ref(xr)
    yr = (yr[0] if isinstance(yr, tuple) else yr).permute(0, 2, 3, 4, 1)
    errs = {"out": l2(y.cpu(), yr)}
    dy = orc.closed_form_tensor(tuple(yr.shape), 77, -1.0, 1.0)
    y.backward(dy.to(DEV))
    yr.backward(dy.double())
    errs["dx"] = l2(xd.grad.cpu(), xr.grad)
    want = dict(ref.named_parameters())
    top = max(float(q.grad.norm()) for q in want.values() if q.grad is not None)
    for k, p in mod.named_parameters():
        if want[k].grad is None or float(want[k].grad.norm()) < 1e-3 * top:
            continue
        errs[k] = l2(p.grad.cpu(), want[k].grad)
    med = float(np.median(list(errs.values())))
    print("s16 embedded TPAVIModule(128):", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["out"] <= 5e-2 and errs["dx"] <= 5e-2 and med <= 5e-2 and max(errs.values()) <= 0.2, errs
    rb = dict(ref.named_buffers())
    for k, b in mod.named_buffers():
        if b.dtype.is_floating_point:
            assert not torch.equal(b.cpu().double(), b0[k]), f"{k} not updated"
            assert l2(b.cpu(), rb[k]) <= 5e-2, k
    # eval mode: running statistics
    mod.eval(); ref.eval()
    with torch.no_grad():
        ye = ops16.to_f32(mod.forward_nvhwc(ops16.to_bf16(x.to(DEV).permute(0, 2, 3, 4, 1).contiguous())))
        yre = ref(x.double())
        yre = (yre[0] if isinstance(yre, tuple) else yre).permute(0, 2, 3, 4, 1)
    assert l2(ye.cpu(), yre) <= 5e-2


def _block_run(mod, x, seed):
    x = x.clone().requires_grad_(True)
    z = mod.forward_nvhwc(x)
    z.backward(torch.randn(z.shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(z.dtype))
    torch.cuda.synchronize()
    return z.detach(), x.grad, {k: p.grad.clone() for k, p in mod.named_parameters() if p.grad is not None}


def test_s16_tpavi_embedded_model_width_vs_f32():
    """TPAVIModule(2048, 'embedded') at N = 2, V = 3, 28 x 28 (L = 2352, Ci = 1024) under bf16 against the same module under f32
    (the fused exact-fp32 attention kernel)."""
    from glfusion_amd import ops
    from glfusion_amd.models.ours import TPAVIModule
    res = {}
    # input scale 0.25: scores of standard deviation ~4 through the kaiming projections (at scale 1 they reach ~64, a one-hot softmax
    # whose gradient bf16 storage of theta / phi alone reorders)
    x = 0.25 * torch.randn(2, 3, 28, 28, 2048, generator=torch.Generator().manual_seed(71))
    for prec in ("f32", "bf16"):
        ops.set_precision(prec)
        mod = TPAVIModule(in_channels=2048, mode="embedded")
        zero_mean_kinkfree_fill(mod, 72)
        mod = mod.to(DEV).train()
        xin = x.to(DEV).to(BF if prec == "bf16" else torch.float32)
        res[prec] = _block_run(mod, xin, 73)
    (z32, dx32, g32), (z16, dx16, g16) = res["f32"], res["bf16"]
    e_out, e_dx = l2(z16.float(), z32.float()), l2(dx16.float(), dx32.float())
    eg = {k: l2(g16[k].float(), g32[k].float()) for k in g32 if float(g32[k].norm()) > 1e-3 * max(float(v.norm()) for v in g32.values())}
    med = float(np.median(list(eg.values())))
    print(f"s16 embedded width 2048: out {e_out:.2e}, dx {e_dx:.2e}, median grad {med:.2e}, worst {max(eg.values()):.2e}")
    assert e_out <= 5e-2 and e_dx <= 5e-2 and med <= 5e-2, (e_out, e_dx, eg)


def test_s16_tpavi_embedded_needs_no_LxL_memory():
    """L = 15,680 (5 views x 56^2): one frame of bf16 scores alone would be 492 MB; the embedded block's peak stays within the 'dot'
    block's + 64 MiB."""
    from glfusion_amd.models.ours import TPAVIModule
    x = torch.randn(8, 5, 56, 56, 2048, generator=torch.Generator().manual_seed(81)).to(BF).to(DEV)
    peaks = {}
    for mode in ("dot", "embedded"):
        mod = TPAVIModule(in_channels=2048, mode=mode)
        zero_mean_kinkfree_fill(mod, 82)
        mod = mod.to(DEV).train()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = _block_run(mod, x, 83)
        peaks[mode] = torch.cuda.max_memory_allocated() - base
        assert bool(torch.isfinite(out[0].float()).all()) and bool(torch.isfinite(out[1].float()).all())
        del mod, out
    print(f"peak above start: dot {peaks['dot'] / 2**20:.0f} MiB, embedded {peaks['embedded'] / 2**20:.0f} MiB")
    assert peaks["embedded"] <= peaks["dot"] + 64 * 2 ** 20, peaks


def test_s16_tpavi_embedded_graph_capture_replays_bitwise():
    from glfusion_amd.models.ours import TPAVIModule
    mod = TPAVIModule(in_channels=256, mode="embedded")
    zero_mean_kinkfree_fill(mod, 91)
    mod = mod.to(DEV).train()
    x = torch.randn(2, 3, 12, 14, 256, generator=torch.Generator().manual_seed(92)).to(DEV).to(BF)
    gz = torch.randn(2, 3, 12, 14, 256, generator=torch.Generator().manual_seed(93)).to(DEV).to(BF)
    xs = x.clone().requires_grad_(True)

    def step():
        xs.grad = None
        for p in mod.parameters():
            p.grad = None
        z = mod.forward_nvhwc(xs)
        z.backward(gz)
        return z

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                              # warm-up on the side stream (caches, workspaces)
    torch.cuda.current_stream().wait_stream(s)
    # eager reference from the same module state (BatchNorm running stats advance each train step: snapshot them)
    buf0 = {k: b.clone() for k, b in mod.named_buffers()}
    z_e = step().detach().clone()
    dx_e = xs.grad.clone()
    g_e = {k: None if p.grad is None else p.grad.clone() for k, p in mod.named_parameters()}
    with torch.no_grad():
        for k, b in mod.named_buffers():
            b.copy_(buf0[k])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z_g = step()
    with torch.no_grad():
        for k, b in mod.named_buffers():
            b.copy_(buf0[k])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(z_g, z_e) and torch.equal(xs.grad, dx_e)
    for k, p in mod.named_parameters():
        assert (p.grad is None and g_e[k] is None) or torch.equal(p.grad, g_e[k]), k
