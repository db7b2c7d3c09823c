"""GPU: the streaming kernels of the U-Net baselines (csrc/unet_ops.hip; glf_conv3x3_c1_*, glf_maxpool2x2s2_*, glf_upsample2x_*,
glf_concat2_* and their glf_s16_* forms) against torch on the CPU in float64.

fp32 storage: the copies and the pool are exact; the sums are within fp32 rounding of the float64 sums -- (k - 1) u sum|terms| for a
chain of k additions, u = 2^-24.  bf16 storage: inputs are bf16-representable, and the result equals the fp32 kernel's rounded once
(torch.equal after .bfloat16()): one kernel body serves both, so the fp32 arithmetic is the same."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
BF = torch.bfloat16
STORAGES = ("f32", "bf16")


def _ops():
    from glfusion_amd import ops
    return ops


def rnd(shape, seed, lo=-1.0, hi=1.0, bf=True):
    g = torch.Generator().manual_seed(seed)
    t = lo + (hi - lo) * torch.rand(shape, generator=g)
    return t.bfloat16().float() if bf else t          # representable in both storages


def ints(shape, seed, hi=3):
    """Small non-negative integers, as after a ReLU: ties in most windows, exact in bf16."""
    return torch.randint(0, hi, shape, generator=torch.Generator().manual_seed(seed)).float()


def dev(t, storage):
    return t.to(DEV).to(BF if storage == "bf16" else torch.float32).contiguous()


def launch(name, ref, *args):
    _ops()._launch(name, ref, *args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ max-pool
def pool_ref(x):
    """x [n,h,w,c] -> (y, idx) with the first maximum in row-major window order; NaN-free inputs."""
    n, h, w, c = x.shape
    ho, wo = h // 2, w // 2
    win = [x[:, ky:2 * ho:2, kx:2 * wo:2] for ky in (0, 1) for kx in (0, 1)]
    best, idx = win[0].clone(), torch.zeros(n, ho, wo, c, dtype=torch.uint8)
    for t in (1, 2, 3):
        m = win[t] > best
        best = torch.where(m, win[t], best)
        idx = torch.where(m, torch.full_like(idx, t), idx)
    return best, idx


def pool_bwd_ref(dy, idx, h, w):
    n, ho, wo, c = dy.shape
    dx = torch.zeros(n, h, w, c, dtype=dy.dtype)
    for t in range(4):
        dx[:, t // 2:2 * ho:2, t % 2:2 * wo:2] = torch.where(idx == t, dy, torch.zeros_like(dy))
    return dx


def run_pool(x, dy, storage):
    n, h, w, c = x.shape
    xd, dyd = dev(x, storage), dev(dy, storage)
    y = torch.empty(n, h // 2, w // 2, c, dtype=xd.dtype, device=DEV)
    idx = torch.empty(n, h // 2, w // 2, c, dtype=torch.uint8, device=DEV)
    launch("maxpool2x2s2_fwd", xd, xd, y, idx, n, h, w, c)
    dx = torch.full((n, h, w, c), float("nan"), dtype=xd.dtype, device=DEV)        # the kernel must write every element
    launch("maxpool2x2s2_bwd", dyd, dyd, idx, dx, n, h, w, c)
    return y.cpu(), idx.cpu(), dx.cpu()


@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", [(2, 7, 5, None), (1, 2, 2, 64), (3, 6, 9, 72)])
def test_maxpool2x2s2(shape, storage):
    n, h, w, c = shape
    c = c or (8 if storage == "bf16" else 4)
    x, dy = ints((n, h, w, c), 1), rnd((n, h // 2, w // 2, c), 2)
    want_y, want_idx = pool_ref(x)
    assert torch.equal(want_y, F.max_pool2d(x.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1))
    assert float((want_idx == 0).float().mean()) > 0.3 and int(want_idx.max()) == 3          # ties and every position occur
    y, idx, dx = run_pool(x, dy, storage)
    assert torch.equal(y.float(), want_y) and torch.equal(idx, want_idx)
    want_dx = pool_bwd_ref(dy, want_idx, h, w)
    assert torch.equal(dx.float(), want_dx)                                    # no NaN left: every element written, zeros included
    if h % 2:
        assert torch.equal(dx[:, h - 1].float(), torch.zeros(n, w, c))
    if w % 2:
        assert torch.equal(dx[:, :, w - 1].float(), torch.zeros(n, h, c))
    # the autograd node gives the same
    ops = _ops()
    xg = dev(x, storage).requires_grad_(True)
    yg = ops.maxpool2x2s2(xg)
    yg.backward(dev(dy, storage))
    torch.cuda.synchronize()
    assert torch.equal(yg.detach().cpu().float(), want_y) and torch.equal(xg.grad.cpu().float(), want_dx)


@pytest.mark.parametrize("storage", STORAGES)
def test_maxpool2x2s2_constant_windows_pick_the_origin(storage):
    n, h, w, c = 2, 7, 5, 8
    x = torch.zeros(n, h, w, c)
    x[:, :6, :4] = ints((n, 3, 2, c), 3, hi=5).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    dy = rnd((n, 3, 2, c), 4).abs() + 0.5
    y, idx, dx = run_pool(x, dy, storage)
    assert int(idx.max()) == 0
    origins = torch.zeros(n, h, w, c, dtype=torch.bool)
    origins[:, 0:6:2, 0:4:2] = True
    assert bool((dx.float() != 0).eq(origins).all())


@pytest.mark.parametrize("storage", STORAGES)
def test_maxpool2x2s2_refusals(storage):
    c = 8
    x = dev(torch.zeros(1, 1, 4, c), storage)
    y = torch.empty(1, 1, 2, c, dtype=x.dtype, device=DEV)
    idx = torch.empty(1, 1, 2, c, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        launch("maxpool2x2s2_fwd", x, x, y, idx, 1, 1, 4, c)
    with pytest.raises(RuntimeError, match="H, W >= 2"):
        launch("maxpool2x2s2_bwd", y, y, idx, x, 1, 1, 4, c)
    with pytest.raises(RuntimeError, match="channel count"):
        launch("maxpool2x2s2_fwd", x, x, y, idx, 1, 2, 2, 6)


# ------------------------------------------------------------------------------------------------------------------ up-sample
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("shape", [(2, 3, 2, None), (1, 1, 1, 64), (2, 7, 14, 72)])
def test_upsample2x(shape, storage):
    n, h, w, c = shape
    c = c or (8 if storage == "bf16" else 4)
    ops = _ops()
    x, dy = rnd((n, h, w, c), 5), rnd((n, 2 * h, 2 * w, c), 6)
    want_y = F.interpolate(x.permute(0, 3, 1, 2).double(), scale_factor=2).permute(0, 2, 3, 1)
    assert torch.equal(want_y, x.double().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2))
    box = dy.double().reshape(n, h, 2, w, 2, c)
    want_dx, mag = box.sum(dim=(2, 4)), box.abs().sum(dim=(2, 4))
    got = {}
    for st in ("f32", storage):
        xg = dev(x, st).requires_grad_(True)
        y = ops.upsample2x(xg)
        y.backward(dev(dy, st))
        torch.cuda.synchronize()
        got[st] = (y.detach().cpu(), xg.grad.cpu())
    assert torch.equal(got["f32"][0].double(), want_y)
    assert bool(((got["f32"][1].double() - want_dx).abs() <= 3 * U * mag).all())
    if storage == "bf16":
        assert got["bf16"][0].dtype == BF and torch.equal(got["bf16"][0], got["f32"][0].bfloat16())
        assert torch.equal(got["bf16"][1], got["f32"][1].bfloat16())


# --------------------------------------------------------------------------------------------------------------------- concat
@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("sliced", [False, True])
@pytest.mark.parametrize("ca,cb", [(4, 12), (64, 64), (8, 24)])
def test_concat2(ca, cb, sliced, storage):
    ops = _ops()
    rows, wd = 30, (8 if storage == "bf16" else 4)
    if sliced:        # both sources are column slices of one wider buffer (row stride ca + cb + 2 accesses)
        wide = dev(rnd((rows, ca + cb + 2 * wd), 7), storage)
        a, b = wide[:, wd:wd + ca], wide[:, wd + ca:wd + ca + cb]
        assert not a.is_contiguous() and not b.is_contiguous()
    else:
        a, b = dev(rnd((rows, ca), 8), storage), dev(rnd((rows, cb), 9), storage)
    if storage == "bf16" and (ca % 8 or cb % 8):          # 16-byte accesses of eight bf16: refused, not mis-copied
        with pytest.raises(RuntimeError, match="multiples of the 16-byte access"):
            ops.concat_channels(a, b)
        return
    ag, bg = a.detach().requires_grad_(True), b.detach().requires_grad_(True)
    y = ops.concat_channels(ag, bg)
    torch.cuda.synchronize()
    want = torch.cat((a.cpu(), b.cpu()), dim=1)
    assert tuple(y.shape) == (rows, ca + cb) and torch.equal(y.detach().cpu(), want)
    y.backward(y.detach())                                 # backward round-trips: the slices of y are the sources
    torch.cuda.synchronize()
    assert ag.grad.is_contiguous() and torch.equal(ag.grad.cpu(), a.cpu()) and torch.equal(bg.grad.cpu(), b.cpu())
    # 4-D, as the models call it
    a4, b4 = a.contiguous().view(2, 3, 5, ca), b.contiguous().view(2, 3, 5, cb)
    assert torch.equal(ops.concat_channels(a4, b4).cpu(), want.view(2, 3, 5, ca + cb))


# ------------------------------------------------------------------------------------------------------------- entry convolution
PIX = 1024        # pixels one workgroup reduces in wgrad (one [10][64] block of partial sums each)
C1_SHAPES = [(3, 1, 1), (2, 5, 7), (2, 48, 32), (1, 33, 31), (1, 32, 32), (1, 25, 41)]      # ..., PIX - 1, PIX, PIX + 1 pixels


def c1_case(n, h, w):
    x = rnd((n, 1, h, w), 10, 0.0, 1.0, bf=False)
    wt, b = rnd((64, 1, 3, 3), 11, -0.8, 0.8, bf=False), rnd((64,), 12, -0.1, 0.1, bf=False)
    dy = rnd((n, h, w, 64), 13)
    return x, wt, b, dy


def c1_run(x, wt, b, dy, storage):
    ops = _ops()
    n, _, h, w = x.shape
    w_ = wt.to(DEV).requires_grad_(True)
    b_ = b.to(DEV).requires_grad_(True)
    with ops.precision_scope("bf16" if storage == "bf16" else "f32"):
        y = ops.conv3x3_c1(x.to(DEV).reshape(n, h, w, 1), w_, b_)
        y.backward(dev(dy, storage))
    torch.cuda.synchronize()
    return y.detach().cpu(), w_.grad.cpu(), b_.grad.cpu()


@pytest.mark.parametrize("shape", C1_SHAPES)
def test_conv3x3_c1(shape):
    n, h, w = shape
    from glfusion_amd._lib import lib
    assert lib.glf_conv3x3_c1_wgrad_workspace(n, h, w, 64) == -(-n * h * w // PIX) * 640
    assert sorted(s[0] * s[1] * s[2] for s in C1_SHAPES)[-4:-1] == [PIX - 1, PIX, PIX + 1]
    x, wt, b, dy = c1_case(n, h, w)
    xd, wd_, dyd = x.double(), wt.double(), dy.double().permute(0, 3, 1, 2)
    want_y = F.conv2d(xd, wd_, b.double(), padding=1).permute(0, 2, 3, 1)
    mag_y = F.conv2d(xd.abs(), wd_.abs(), b.double().abs(), padding=1).permute(0, 2, 3, 1)
    patches = F.unfold(xd, 3, padding=1)                                       # [n, 9, h*w]
    want_dw = torch.einsum("nco,nto->ct", dyd.reshape(n, 64, -1), patches).reshape(64, 1, 3, 3)
    mag_dw = torch.einsum("nco,nto->ct", dyd.reshape(n, 64, -1).abs(), patches.abs()).reshape(64, 1, 3, 3)
    want_db, mag_db = dyd.sum(dim=(0, 2, 3)), dyd.abs().sum(dim=(0, 2, 3))
    y, dw, db = c1_run(x, wt, b, dy, "f32")
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, h, w, 64)
    assert bool(((y.double() - want_y).abs() <= 10 * U * mag_y).all())          # bias + 9 fused multiply-adds
    # a thread adds at most PIX / 16 products in fp32 (16 pixel lanes; 32 under bf16), the lanes and the four wavefronts meet in <= 5
    # more fp32 additions, the blocks in float64, one rounding at the end
    k = PIX // 16 + 8
    assert bool(((dw.double() - want_dw).abs() <= k * U * mag_dw).all()), float(((dw.double() - want_dw).abs() / mag_dw.clamp_min(1e-30)).max())
    assert bool(((db.double() - want_db).abs() <= k * U * mag_db).all())
    # no atomics: the same call again gives the same bits
    y2, dw2, db2 = c1_run(x, wt, b, dy, "f32")
    assert torch.equal(y, y2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    # bf16 storage: the output is the fp32 one rounded once; the gradients are fp32 either way and sum the same dy over other pixel
    # lanes (eight channels per thread): the same bound against float64
    y16, dw16, db16 = c1_run(x, wt, b, dy, "bf16")
    assert y16.dtype == BF and torch.equal(y16, y.bfloat16())
    assert dw16.dtype == torch.float32 and bool(((dw16.double() - want_dw).abs() <= k * U * mag_dw).all())
    assert bool(((db16.double() - want_db).abs() <= k * U * mag_db).all())
    y16b, dw16b, db16b = c1_run(x, wt, b, dy, "bf16")
    assert torch.equal(y16, y16b) and torch.equal(dw16, dw16b) and torch.equal(db16, db16b)


@pytest.mark.parametrize("storage", STORAGES)
def test_conv3x3_c1_refusals(storage):
    from glfusion_amd._lib import lib
    ops = _ops()
    n, h, w = 2, 48, 32
    x, wt, b, dy = c1_case(n, h, w)
    xd, dyd = x.to(DEV), dev(dy, storage)
    dw, db = torch.empty(64, 9, device=DEV), torch.empty(64, device=DEV)
    need = int(lib.glf_conv3x3_c1_wgrad_workspace(n, h, w, 64))
    part = torch.empty(need, device=DEV)
    launch("conv3x3_c1_wgrad", dyd, xd, dyd, dw, db, part, need, n, h, w, 64)
    with pytest.raises(RuntimeError, match="workspace"):
        launch("conv3x3_c1_wgrad", dyd, xd, dyd, dw, db, part, need - 1, n, h, w, 64)
    y = torch.empty(n, h, w, 32, dtype=dyd.dtype, device=DEV)
    with pytest.raises(RuntimeError, match="Cout must be 64"):
        launch("conv3x3_c1_fwd", y, xd, wt[:32].contiguous().to(DEV), None, y, n, h, w, 32)
    # no dgrad: the image's gradient is not on the path
    xg = xd.reshape(n, h, w, 1).requires_grad_(True)
    with ops.precision_scope("bf16" if storage == "bf16" else "f32"):
        out = ops.conv3x3_c1(xg, wt.to(DEV).requires_grad_(True), None)
        with pytest.raises(RuntimeError, match="gradient w.r.t. the input image is not on the path"):
            out.backward(dyd)
