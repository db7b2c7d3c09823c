"""Host plan of the segmented region mode (glf_gemm_nt_seg_plan, include/glfusion.h) against a brute-force evaluation per pixel.

No GPU: the plan function is host code of libglfusion_hip.so, called through ctypes.  For maps h, w in {1, 5, 9, 12, 28} and
segment lists built like ops.aspp_dgrad_segments builds them (the eight off-centre taps of a 3x3 kernel per dilation, offsets
((1 - ky) d, (1 - kx) d)) from dilation sets drawn from {1, 2, 3, 6, 7, 12, 24, 36}, every plan must
  * partition the map: every pixel lies in exactly one rectangle;
  * give every rectangle the segment mask that equals the in-range set of EVERY one of its pixels;
  * report row-tile counts that are ceil(n_img * area / 256) per rectangle and sum to the launcher's grid figure;
  * list the rectangles in non-increasing order of segment count."""
import ctypes
import itertools

import numpy as np
import pytest

from glfusion_amd import _lib

SIZES = (1, 5, 9, 12, 28)
DILS = (1, 2, 3, 6, 7, 12, 24, 36)
# every single dilation, the model's set, the GPU tests' sets, and a spread of triples (three distinct |offset| values per axis
# is the most the plan takes: 7 bands)
DIL_SETS = [(d,) for d in DILS] + [(12, 24, 36), (2, 4, 7), (3, 6, 12), (1, 2, 3), (6, 7, 12), (1, 7, 24), (2, 12, 36), (3, 24), (7, 36)]


def _segments(dils, cout=32):
    segs = []
    for i, d in enumerate(dils, start=1):
        for t in range(9):
            if t != 4:
                ky, kx = divmod(t, 3)
                segs.append(((1 - ky) * d, (1 - kx) * d, i * cout))
    return segs


def _plan(n_img, h, w, segs):
    dll = _lib.lib.load()
    arr = (ctypes.c_int32 * (3 * len(segs)))(*[v for s in segs for v in s])
    regions = (ctypes.c_int32 * (6 * _lib.SEG_MAX_REGIONS))()
    nreg, tiles = ctypes.c_int32(0), ctypes.c_int64(0)
    rc = dll.glf_gemm_nt_seg_plan(n_img, h, w, len(segs), ctypes.cast(arr, ctypes.c_void_p), ctypes.cast(regions, ctypes.c_void_p),
                                  ctypes.cast(ctypes.pointer(nreg), ctypes.c_void_p), ctypes.cast(ctypes.pointer(tiles), ctypes.c_void_p))
    return rc, np.array(regions[:6 * nreg.value], dtype=np.int64).reshape(-1, 6), int(tiles.value)


def _brute_masks(h, w, segs):
    """[h][w] bit mask of the segments whose shifted pixel lies inside the map."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    m = np.zeros((h, w), dtype=np.int64)
    for s, (oy, ox, _) in enumerate(segs):
        ok = (yy + oy >= 0) & (yy + oy < h) & (xx + ox >= 0) & (xx + ox < w)
        m |= ok.astype(np.int64) << s
    return m


@pytest.mark.parametrize("dils", DIL_SETS, ids=lambda d: "-".join(map(str, d)))
def test_plan_matches_brute_force(dils):
    segs = _segments(dils)
    assert len(segs) <= _lib.SEG_MAX
    for h, w, n_img in itertools.product(SIZES, SIZES, (1, 3)):
        rc, regions, tiles = _plan(n_img, h, w, segs)
        assert rc == 0, (h, w, dils)
        assert 1 <= len(regions) <= _lib.SEG_MAX_REGIONS
        want = _brute_masks(h, w, segs)
        cover = np.zeros((h, w), dtype=np.int64)
        total, counts = 0, []
        for y0, y1, x0, x1, mask, rt in regions:
            assert 0 <= y0 < y1 <= h and 0 <= x0 < x1 <= w, (h, w, dils)
            cover[y0:y1, x0:x1] += 1
            assert (want[y0:y1, x0:x1] == mask).all(), (h, w, dils, (y0, y1, x0, x1))
            assert rt == -(-(n_img * (y1 - y0) * (x1 - x0)) // _lib.SEG_ROW_TILE)
            total += rt
            counts.append(bin(mask).count("1"))
        assert (cover == 1).all(), (h, w, dils)
        assert total == tiles
        assert counts == sorted(counts, reverse=True)


def test_plan_refuses_what_the_kernel_does_not_take():
    # more than three distinct |offset| values on an axis: more than 7 bands
    rc, _, _ = _plan(1, 28, 28, _segments((1, 2, 3))[:8] + [(5, 0, 0), (9, 0, 0), (13, 0, 0)])
    assert rc != 0
    # more segments than a 32-bit mask with the documented bound takes
    rc, _, _ = _plan(1, 28, 28, [(1, 0, 0)] * (_lib.SEG_MAX + 1))
    assert rc != 0


def test_params_mirror_has_the_segment_fields_last():
    names = [f[0] for f in _lib.GemmParams._fields_]
    assert names[-3:] == ["nseg", "seg_kx", "seg"]
    assert ctypes.sizeof(_lib.GemmParams) == _lib.lib.load().glf_sizeof_gemm_params()
