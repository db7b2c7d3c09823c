"""Host plan of a segmented launch whose segments belong to groups of output columns (glf_gemm_nt_seg_plan_cols,
include/glfusion.h) and the weight-image contract of ops.aspp_fwd_weights / ops.aspp_fwd_cols, without a GPU.

The plan is host code of libglfusion_hip.so, called through ctypes.  For the shapes of tests/test_gpu_aspp_fwd_one.py, the
model's head and a few more:
  * for EVERY pixel and EVERY column tile, `mask of the pixel's rectangle & mask of the column tile` is the set brute force gives:
    the taps of the branch that owns the tile whose shifted pixel lies inside the map, and nothing for the 1x1 branch's tiles;
  * the dispatch list names every (rectangle, row tile, column tile) once, its chain lengths do not increase from one run of 16
    entries to the next, and the work it hands to the eight XCDs (blockIdx % 8) differs by less than two of the longest chains;
  * column ranges that are not whole 128-column tiles, or more column tiles than the table holds, are refused;
  * the B offsets of aspp_fwd_cols address, inside the torch.cat of the weight slices that aspp_fwd_weights' image is, exactly the
    tap slab of each segment for each column of its branch;
  * glf_gemm_params did not grow: the column groups travel as arguments of glf_gemm_nt_seg_cols."""
import ctypes

import numpy as np
import pytest
import torch

from glfusion_amd import _lib

COL_TILE = 128
# (n, h, w, Cout, rates): the GPU test's three shapes, the model's head, one branch per column tile pair, and tiny maps
SHAPES = [(2, 9, 12, 128, (2, 4, 7)), (3, 28, 28, 128, (12, 24, 36)), (2, 12, 10, 128, (3, 6, 12)), (64, 28, 28, 256, (12, 24, 36)),
          (1, 5, 5, 256, (1, 2, 3)), (3, 1, 9, 128, (1, 7)), (1, 28, 12, 384, (6,))]


def _ptr(x):
    return ctypes.cast(x, ctypes.c_void_p)


def _plan(n_img, h, w, segs, cols, N, want_order=True):
    dll = _lib.lib.load()
    ns = len(segs)
    seg = (ctypes.c_int32 * (3 * ns))(*[v for _, _, oy, ox, _ in segs for v in (oy, ox, 0)])
    ca = (ctypes.c_int32 * (2 * ns))(*[v for c in cols for v in c[:2]])
    regions = (ctypes.c_int32 * (6 * _lib.SEG_MAX_REGIONS))()
    nreg, tiles = ctypes.c_int32(0), ctypes.c_int64(0)
    tiles_n = -(-N // COL_TILE)
    masks = (ctypes.c_uint32 * max(tiles_n, 64))()
    cap = 1 << 16
    order = (ctypes.c_int32 * (3 * cap))()
    rc = dll.glf_gemm_nt_seg_plan_cols(n_img, h, w, ns, _ptr(seg), _ptr(ca), N, _ptr(regions), _ptr(ctypes.pointer(nreg)),
                                       _ptr(ctypes.pointer(tiles)), _ptr(masks), _ptr(order) if want_order else None, cap)
    if rc != 0:
        return rc, None, 0, None, None
    units = int(tiles.value) * tiles_n
    return (rc, np.array(regions[:6 * nreg.value], dtype=np.int64).reshape(-1, 6), int(tiles.value),
            np.array(masks[:tiles_n], dtype=np.int64), np.array(order[:3 * units], dtype=np.int64).reshape(-1, 3))


def _head(h, w, cout, rates):
    from glfusion_amd import ops
    segs = ops.aspp_fwd_segments(rates, h, w, cout)
    return segs, ops.aspp_fwd_cols(segs, 1 + len(rates), cout, 64)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:4])) + "-" + "-".join(map(str, s[4])))
def test_segment_set_of_every_pixel_and_column_tile(shape):
    n, h, w, cout, rates = shape
    k = 1 + len(rates)
    N = k * cout
    segs, cols = _head(h, w, cout, rates)
    assert 0 < len(segs) <= _lib.SEG_MAX
    # the segment list itself: every off-centre tap of every dilated branch that is in range for some pixel, branch by branch
    brute = [(i, t, (t // 3 - 1) * d, (t % 3 - 1) * d, i * cout) for i, d in enumerate(rates, start=1) for t in range(9)
             if t != 4 and abs((t // 3 - 1) * d) < h and abs((t % 3 - 1) * d) < w]
    assert segs == brute
    rc, regions, tiles, masks, order = _plan(n, h, w, segs, cols, N)
    assert rc == 0
    region_of = -np.ones((h, w), dtype=np.int64)
    for r, (y0, y1, x0, x1, _, _) in enumerate(regions):
        assert (region_of[y0:y1, x0:x1] == -1).all()
        region_of[y0:y1, x0:x1] = r
    assert (region_of >= 0).all()
    for tn in range(N // COL_TILE):
        branch = tn * COL_TILE // cout
        for y in range(h):
            for x in range(w):
                want = 0
                for s, (i, _, oy, ox, _) in enumerate(segs):
                    if i == branch and 0 <= y + oy < h and 0 <= x + ox < w:
                        want |= 1 << s
                got = int(regions[region_of[y, x]][4]) & int(masks[tn])
                assert got == want, (shape, tn, y, x, bin(got), bin(want))
        if branch == 0:
            assert masks[tn] == 0
    # the dispatch list: a permutation of the workgroups, longest chains first, the XCDs' shares balanced
    assert len(order) == tiles * (N // COL_TILE)
    every = {(r, tm, tn) for r, reg in enumerate(regions) for tm in range(int(reg[5])) for tn in range(N // COL_TILE)}
    assert {tuple(int(v) for v in e) for e in order} == every and len(every) == len(order)
    chain = np.array([bin(int(regions[r][4]) & int(masks[tn])).count("1") for r, _, tn in order])
    runs = [chain[i:i + 16] for i in range(0, len(chain), 16)]
    for a, b in zip(runs, runs[1:]):
        assert a.min() >= b.max(), shape
    # (heaviest pair to the least-loaded XCD keeps the spread within one pair's weight; the last, partial run adds at most two of
    # the shortest workgroups to an XCD)
    load = [int((1 + chain[x::8]).sum()) for x in range(8)]
    assert max(load) - min(load) <= 2 * (1 + int(chain.max())) + 2 * (1 + int(chain[-1])), (shape, load)


def test_plan_refuses_what_the_kernel_does_not_take():
    segs, cols = _head(28, 28, 128, (12, 24, 36))
    assert _plan(2, 28, 28, segs, cols, 512)[0] == 0
    bad = [(c0 + 64, cn, b) for c0, cn, b in cols]                       # not on a tile boundary
    assert _plan(2, 28, 28, segs, bad, 512)[0] != 0
    bad = [(c0, 96, b) for c0, cn, b in cols]                            # not whole tiles
    assert _plan(2, 28, 28, segs, bad, 512)[0] != 0
    bad = [(c0 + 256, cn, b) for c0, cn, b in cols]                      # past N
    assert _plan(2, 28, 28, segs, bad, 512)[0] != 0
    wide = [(c0, cn, b) for c0, cn, b in cols]
    assert _plan(2, 28, 28, segs, wide, 65 * COL_TILE)[0] != 0           # more column tiles than the table holds
    assert _plan(2, 28, 28, segs, cols, 512, want_order=False)[0] == 0   # the list is optional


@pytest.mark.parametrize("shape", [(9, 12, 128, (2, 4, 7)), (28, 28, 256, (12, 24, 36))], ids=["9x12", "28x28"])
def test_b_offsets_address_the_tap_slabs_of_the_stacked_image(shape):
    from glfusion_amd import ops
    h, w, cout, rates = shape
    cin, k = 32, 1 + len(rates)
    g = torch.Generator().manual_seed(3)
    ws = [torch.randn(cout, cin, 1, 1, generator=g)] + [torch.randn(cout, cin, 3, 3, generator=g) for _ in rates]
    segs = ops.aspp_fwd_segments(rates, h, w, cout)
    cols = ops.aspp_fwd_cols(segs, k, cout, cin)
    # what ops.aspp_fwd_weights builds (tests/test_gpu_aspp_fwd_one.py compares the device image with this torch.cat bit for bit)
    image = torch.cat([ws[0][:, :, 0, 0]] + [t[:, :, 1, 1] for t in ws[1:]] + [ws[i][:, :, t // 3, t % 3] for i, t, _, _, _ in segs], dim=0)
    assert tuple(image.shape) == ((k + len(segs)) * cout, cin)
    flat = image.reshape(-1)
    for (i, t, oy, ox, col0), (c0, cn, boff) in zip(segs, cols):
        assert (c0, cn) == (i * cout, cout) == (col0, cout) and boff % 4 == 0 and boff >= 0
        assert (oy, ox) == ((t // 3 - 1) * rates[i - 1], (t % 3 - 1) * rates[i - 1])
        for c in (c0, c0 + 1, c0 + cn - 1):
            got = flat[c * cin + boff:c * cin + boff + cin]
            assert torch.equal(got, ws[i][c - c0, :, t // 3, t % 3]), (i, t, c)
    # the K columns of every row: the 1x1 weight and the centre taps
    assert torch.equal(image[:cout], ws[0][:, :, 0, 0]) and all(torch.equal(image[i * cout:(i + 1) * cout], ws[i][:, :, 1, 1]) for i in range(1, k))


def test_params_mirror_did_not_grow():
    names = [f[0] for f in _lib.GemmParams._fields_]
    assert names[-3:] == ["nseg", "seg_kx", "seg"]
    dll = _lib.lib.load()
    assert ctypes.sizeof(_lib.GemmParams) == dll.glf_sizeof_gemm_params() and dll.glf_abi_version() == 7
    protos = _lib.parse_header()
    assert protos["glf_gemm_nt_seg_cols"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(_lib.GemmParams),
                                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p])
    assert "glf_gemm_nt_seg_plan_cols" in protos
