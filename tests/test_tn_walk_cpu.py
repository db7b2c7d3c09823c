"""CPU: the host side of the TN slice rule (csrc/gemm_tn_walk.h) through the two entry points that size the partial-sum
workspace, glf_gemm_tn_workspace_bytes and glf_s16_gemm_tn_workspace_bytes, against a restatement in Python over a small
exhaustive grid: maps up to 12 x 12, stride 1 and 2, dilation 1..6, every split 1..12, a few tap masks, both batch sizes and the
rectangle form of the bf16-storage entry point (which keeps only the slabs of the slices that run)."""
import ctypes as C
import itertools

from glfusion_amd._lib import GemmParams, lib

S16_KTILE = 64                  # K tile of the bf16-storage TN kernel (the fp32-storage kernels' 32 does not enter a workspace size)
MASKS = [0x1FF, 0x1EF, 0x010, 0x145, 0x0AA]


def valid_slices(rows, K, split, ktile):
    """The slice rule: slices are cut from the FULL reduction length K, rounded up to the K tile; a tap whose rectangle has
    `rows` reduction rows runs the first ceil(rows / chunk) of them."""
    chunk = -(-(-(-K // split)) // ktile) * ktile
    return min(split, -(-rows // chunk))


def band(o, stride, hs, hd):
    """number of output pixels y in [0, hd) whose source pixel y * stride + o lies inside [0, hs), by enumeration"""
    return sum(1 for y in range(hd) if 0 <= y * stride + o < hs)


def rect_rows(n_img, hs, ws, hd, wd, stride, pad, dil, tap):
    ky, kx = divmod(tap, 3)
    return n_img * band(ky * dil - pad, stride, hs, hd) * band(kx * dil - pad, stride, ws, wd)


def params(M, N, n_img, hs, ws, hd, wd, stride, pad, dil, mask, split, batch, rect):
    p = GemmParams()
    p.M, p.N, p.K, p.lda, p.ldb, p.ldc = M, N, n_img * hd * wd, M, N, N
    p.taps, p.tap_mask, p.tap_stride_b, p.gather = 9, mask, M * N, 1
    (p.n_img, p.hs, p.ws, p.hd, p.wd, p.kh, p.kw, p.stride, p.pad, p.dil) = (n_img, hs, ws, hd, wd, 3, 3, stride, pad, dil)
    p.batch, p.alpha, p.split, p.rect = batch, 1.0, split, rect
    return p


def grid():
    for hs, stride, dil in itertools.product(range(1, 13), (1, 2), range(1, 7)):
        for ws in {hs, 13 - hs}:
            for pad in {dil, 0, 1}:
                hd, wd = (hs + 2 * pad - 2 * dil - 1) // stride + 1, (ws + 2 * pad - 2 * dil - 1) // stride + 1
                if hd > 0 and wd > 0:
                    yield hs, ws, hd, wd, stride, pad, dil


def test_workspace_bytes_follow_the_slice_rule():
    lib.glf_gemm_tn_workspace_bytes.restype = lib.glf_s16_gemm_tn_workspace_bytes.restype = C.c_size_t
    M, N, checked, short = 24, 40, 0, 0
    for hs, ws, hd, wd, stride, pad, dil in grid():
        for n_img, mask, split in itertools.product((1, 2), MASKS, range(1, 13)):
            K, ntap = n_img * hd * wd, bin(mask).count("1")
            for batch in (1, 3):
                p = params(M, N, n_img, hs, ws, hd, wd, stride, pad, dil, mask, split, batch, 0)
                dense = 0 if split <= 1 else batch * split * ntap * M * N * 4
                assert lib.glf_gemm_tn_workspace_bytes(C.byref(p)) == dense
                assert lib.glf_s16_gemm_tn_workspace_bytes(C.byref(p)) == dense
                p.c_oihw = 1                                     # the parameter-layout store goes through the workspace at split 1 too
                assert lib.glf_gemm_tn_workspace_bytes(C.byref(p)) == batch * split * ntap * M * N * 4
            # the rectangle form of the bf16-storage entry point: the slabs of the slices that run, tap after tap
            p = params(M, N, n_img, hs, ws, hd, wd, stride, pad, dil, mask, split, 1, 1)
            slabs = sum(valid_slices(rect_rows(n_img, hs, ws, hd, wd, stride, pad, dil, t), K, split, S16_KTILE) for t in range(9) if (mask >> t) & 1)
            assert lib.glf_s16_gemm_tn_workspace_bytes(C.byref(p)) == (0 if split <= 1 else slabs * M * N * 4), (hs, ws, stride, pad, dil, n_img, mask, split)
            assert lib.glf_gemm_tn_workspace_bytes(C.byref(p)) == (0 if split <= 1 else split * ntap * M * N * 4)     # (its slabs are not compacted)
            checked += 1
            short += split > 1 and slabs < split * ntap
    assert checked > 10000 and short > 1000                      # the grid does reach taps that leave slices empty


def test_slice_rule_of_the_issue_examples():
    """K = 100, split 3 at the 32-row tile: chunk 64, two slices run.  Dilation 5 on 2 x 12 x 12 (K = 288), split 4: chunk 96; the
    centre tap runs 3 slices, the edge taps (168 rows) and the corner taps (98 rows) 2."""
    assert valid_slices(100, 100, 3, 32) == 2
    assert valid_slices(33 * 32 + 1, 33 * 32 + 1, 9, 32) == 9 and valid_slices(33 * 32 + 1, 33 * 32 + 1, 33, 32) == 17
    rows = [rect_rows(2, 12, 12, 12, 12, 1, 5, 5, t) for t in range(9)]
    assert rows == [98, 168, 98, 168, 288, 168, 98, 168, 98]
    assert [valid_slices(r, 288, 4, 32) for r in rows] == [2, 2, 2, 2, 3, 2, 2, 2, 2]
