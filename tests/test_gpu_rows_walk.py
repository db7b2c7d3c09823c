"""Edge shapes of the split-fp16 NT kernels' tile walk, row state and output epilogue (csrc/gemm_rows_walk.h), through direct
ops.gemm calls with gather / rect / mask combinations no other test makes.  Every case runs on both tile configurations: the
launcher takes the 4-wave 128-row kernel when K x popcount(tap_mask) <= 256 and the 8-wave 256-row kernel above.  Gate: float64,
the elementwise 5e-5 of test_gpu_ops.py (its `close`)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
NO_CENTRE = 0x1EF               # a 3x3 tap mask with the centre tap cleared: 8 taps x K = 32 = 256 -> 4-wave; x K = 64 -> 8-wave
# (K, rows of a tile of the kernel that K x 8 taps -- or K alone for the plain calls -- selects)
BOTH_3X3 = [(32, 128), (64, 256)]
BOTH_PLAIN = [(32, 128), (288, 256)]


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g) * 2 - 1


def close(a, b, tol=5e-5):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    err = (a - b).abs()
    ok = bool((err <= tol + tol * b.abs()).all())
    if not ok:
        print("max abs err", float(err.max()), "max |ref|", float(b.abs().max()), "tol", tol)
    return ok


@pytest.fixture
def ops():
    from glfusion_amd import ops as _ops
    _ops.set_precision("f16x3")
    yield _ops
    _ops.set_precision("f32")


def conv_out(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


def geo_of(gather, conv):
    """(n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil) of conv = (n, h, w, k, stride, pad, dil): gather 1 maps output pixels to
    input pixels (forward), gather 2 input pixels to output-gradient pixels (dgrad)."""
    n, h, w, k, stride, pad, dil = conv
    ho, wo = conv_out(h, k, stride, pad, dil), conv_out(w, k, stride, pad, dil)
    return (n, h, w, ho, wo, k, k, stride, pad, dil) if gather == 1 else (n, ho, wo, h, w, k, k, stride, pad, dil)


def src_index(gather, geo):
    """[taps][rows]: source row of every destination row and tap, -1 where the tap falls into the padding."""
    n_img, hs, ws, hd, wd, kh, kw, stride, pad, dil = geo
    m = torch.arange(n_img * hd * wd)
    n, y, x = m // (hd * wd), (m // wd) % hd, m % wd
    out = []
    for t in range(kh * kw):
        ky, kx = divmod(t, kw)
        if gather == 1:
            sy, sx = y * stride - pad + ky * dil, x * stride - pad + kx * dil
            ok = (sy >= 0) & (sy < hs) & (sx >= 0) & (sx < ws)
        else:
            ny, nx = y + pad - ky * dil, x + pad - kx * dil
            ok = (ny >= 0) & (nx >= 0) & (ny % stride == 0) & (nx % stride == 0)
            sy, sx = torch.div(ny, stride, rounding_mode="floor"), torch.div(nx, stride, rounding_mode="floor")
            ok = ok & (sy < hs) & (sx < ws)
        out.append(torch.where(ok, (n * hs + sy) * ws + sx, torch.full_like(m, -1)))
    return torch.stack(out)


def gathered_ref(A, B, src, mask):
    """float64 sum over the kept taps of A[src_tap] @ B_tap^T (zero rows in the padding); A [rows][K], B [taps][N][K]."""
    Az = torch.cat([A.double(), torch.zeros(1, A.shape[1], dtype=torch.float64)])
    P = torch.zeros(src.shape[1], B.shape[1], dtype=torch.float64)
    for t in range(B.shape[0]):
        if (mask >> t) & 1:
            P += Az[src[t]] @ B[t].double().T
    return P


def gather_call(ops, gather, conv, K, N, mask, rect=0, accumulate=False, cold=None, seed=0):
    geo = geo_of(gather, conv)
    src = src_index(gather, geo)
    M, rows_a = geo[0] * geo[3] * geo[4], geo[0] * geo[1] * geo[2]
    A, B = rnd(rows_a, K, seed=seed + 1), rnd(9, N, K, seed=seed + 2) / 3
    c = cold.to(DEV).clone() if cold is not None else torch.zeros(M, N, device=DEV)
    ops.gemm("nt", A.to(DEV), B.to(DEV), c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, taps=9, mask=mask, tap_stride_b=N * K, gather=gather,
             geo=geo, rect=rect, accumulate=accumulate)
    ref = gathered_ref(A, B, src, mask) + (cold.double() if (cold is not None and accumulate) else 0.0)
    return c, ref, src


@pytest.mark.parametrize("K,tile", BOTH_3X3)
@pytest.mark.parametrize("gather", [1, 2])
def test_fast_gather_with_tap_census(ops, gather, K, tile):
    """3x3, stride 1, pad = dil = 12 on one 28x28 image, rect = 0: a tile covers fewer than 13 image rows, so the census runs
    and drops the taps that are padding for all of the tile's rows; 784 rows end in a ragged tile of both heights."""
    assert tile < 28 * 13 and 784 % tile != 0
    c, ref, _ = gather_call(ops, gather, (1, 28, 28, 3, 1, 12, 12), K, 72, NO_CENTRE)
    assert close(c, ref)


@pytest.mark.parametrize("K,tile", BOTH_3X3)
def test_strided_dgrad_takes_the_map_src_form(ops, K, tile):
    """gather = 2 of a stride-2 conv (55 -> 28): the only gather that is not the fast (source index + uniform offset) form."""
    c, ref, _ = gather_call(ops, 2, (1, 55, 55, 3, 2, 1, 1), K, 72, NO_CENTRE)
    assert c.shape[0] == 55 * 55 and c.shape[0] % tile != 0
    assert close(c, ref)


# pad = dil = 12 on 28x28: bands [0, 12), [12, 16), [16, 28) per axis.  The first corner region (y, x < 12) reaches the taps
# ky, kx in {1, 2} of a forward gather (bits 4, 5, 7, 8) and ky, kx in {0, 1} of a transposed one (bits 0, 1, 3, 4): clearing
# them leaves that region without taps, while every other region keeps at least one.
REGION_MASK = {1: 0x1FF & ~((1 << 4) | (1 << 5) | (1 << 7) | (1 << 8)), 2: 0x1FF & ~((1 << 0) | (1 << 1) | (1 << 3) | (1 << 4))}


@pytest.mark.parametrize("K,tile", [(32, 128), (64, 256)])          # 5 kept taps: 160 <= 256 < 320
@pytest.mark.parametrize("gather", [1, 2])
def test_region_mode_accumulates_and_leaves_an_empty_region_alone(ops, gather, K, tile):
    """rect = 2 with accumulate onto a non-zero C: every region ends in a ragged tile (144, 48, 16 rows), and the rows of the
    region that has no tap under the mask keep their old values (the split-fp16 walk gives it no tiles)."""
    mask = REGION_MASK[gather]
    assert bin(mask).count("1") == 5
    cold = rnd(784, 72, seed=9)
    c, ref, src = gather_call(ops, gather, (1, 28, 28, 3, 1, 12, 12), K, 72, mask, rect=2, accumulate=True, cold=cold)
    empty = torch.stack([src[t] < 0 for t in range(9) if (mask >> t) & 1]).all(0)
    assert int(empty.sum()) == 144                     # the 12 x 12 corner
    assert torch.equal(c.cpu()[empty], cold[empty])
    assert close(c, ref)


@pytest.mark.parametrize("K,tile", BOTH_3X3)
@pytest.mark.parametrize("gather", [1, 2])
def test_per_tap_rectangles_into_zero_filled_c(ops, gather, K, tile):
    """rect = 1, pad = dil = 24 on 28x28: every kept tap is its own GEMM over its 4-row / 4-column rectangle, summed with float
    atomics into a zero-filled C."""
    c, ref, _ = gather_call(ops, gather, (1, 28, 28, 3, 1, 24, 24), K, 72, NO_CENTRE, rect=1)
    assert close(c, ref)


@pytest.mark.parametrize("K,tile", BOTH_PLAIN)
@pytest.mark.parametrize("rows_over", [3, None])          # 2 tiles + 3 rows: every wave row and two workgroups; one tile: one workgroup
def test_column_statistics_maxima_and_amax(ops, K, tile, rows_over):
    M, N = (2 * tile + rows_over) if rows_over else tile - 5, 132
    A, B, bias = rnd(M, K, seed=41), rnd(N, K, seed=42), rnd(N, seed=43)
    c = torch.empty(M, N, device=DEV)
    stats = torch.zeros(2, N, dtype=torch.float64, device=DEV)
    cmax = torch.zeros(N, device=DEV)
    slot = ops.amax_slot(torch.device(DEV))
    ops.gemm("nt", A.to(DEV), B.to(DEV), c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias.to(DEV), colstats=stats, colmax=cmax, amax_c=slot)
    ref = A.double() @ B.double().T + bias.double()
    assert close(c, ref)
    got = c.double().cpu()                                # the statistics are those of the values stored
    assert torch.allclose(stats[0].cpu(), got.sum(0), rtol=1e-6, atol=1e-6 * float(got.abs().sum(0).max()))
    assert torch.allclose(stats[1].cpu(), (got * got).sum(0), rtol=1e-6)
    assert torch.equal(cmax.cpu(), c.abs().amax(0).cpu())
    assert float(slot) == float(c.abs().max())


@pytest.mark.parametrize("K,tile", BOTH_PLAIN)
def test_fused_epilogue_residual_stride_and_relu(ops, K, tile):
    """The EPI instantiations: residual rows with their own stride (ld_res != ldc), ReLU on, ragged M, N = 132."""
    M, N, ldr = tile + 1, 132, 140
    A, B, bias, res = rnd(M, K, seed=51), rnd(N, K, seed=52), rnd(N, seed=53), rnd(M, ldr, seed=54)
    c = torch.empty(M, N, device=DEV)
    ops.gemm("nt", A.to(DEV), B.to(DEV), c, M=M, N=N, K=K, lda=K, ldb=K, ldc=N, bias=bias.to(DEV), epilogue=(res.to(DEV), ldr, True))
    ref = torch.relu(A.double() @ B.double().T + bias.double() + res[:, :N].double())
    assert close(c, ref)
    assert bool((c == 0).any()) and bool((c > 0).any())
