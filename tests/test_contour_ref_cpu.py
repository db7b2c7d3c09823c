"""CPU: the numpy restatement of the contour metrics (tests/contour_ref.py) against scipy and against hand-made planes."""
import numpy as np
import pytest

import contour_ref as R

PLANES = [(1, 1), (1, 7), (7, 1), (5, 9), (23, 17), (67, 45)]


def _pairs():
    rng = np.random.default_rng(11)
    for h, w in PLANES:
        for density in (0.05, 0.5, 0.95):
            a, b = rng.random((h, w)) < density, rng.random((h, w)) < density
            if a.any() and b.any():
                yield a, b


def test_contour_is_mask_xor_erosion():
    ndi = pytest.importorskip("scipy.ndimage")
    for a, b in _pairs():
        for m in (a, b, np.ones_like(a), np.zeros_like(a)):
            assert np.array_equal(R.contour(m), m ^ ndi.binary_erosion(m))


def test_directed_d2_is_the_exact_distance_transform():
    ndi = pytest.importorskip("scipy.ndimage")
    for a, b in _pairs():
        ea, eb = R.contour(a), R.contour(b)
        for src, dst in ((ea, eb), (eb, ea)):
            edt = ndi.distance_transform_edt(~dst)
            assert np.array_equal(R.directed_d2(src, dst), np.rint(edt[src] ** 2).astype(np.int64))
            assert np.array_equal(R.directed_d2(src, dst, chunk_bytes=64), R.directed_d2(src, dst))      # chunking changes nothing


@pytest.mark.parametrize("pct", [0, 50, 95, 100])
def test_percentile_is_numpys(pct):
    ndi = pytest.importorskip("scipy.ndimage")
    for a, b in _pairs():
        stats, _ = R.plane_stats(a, b, pct)
        p = R.directed_percentile(stats, pct)
        ea, eb = R.contour(a), R.contour(b)
        for d, (src, dst) in enumerate(((ea, eb), (eb, ea))):
            want = np.percentile(ndi.distance_transform_edt(~dst)[src], pct)
            assert abs(p[d] - want) <= 1e-12 * max(abs(want), 1e-300), (a.shape, pct, d, p[d], want)


def test_two_single_pixels_in_opposite_corners():
    a, b = np.zeros((5, 9), bool), np.zeros((5, 9), bool)
    a[0, 0], b[4, 8] = True, True
    stats, sums = R.plane_stats(a, b)
    assert stats.tolist() == [[1, 80, 80, 80], [1, 80, 80, 80]]                    # HD^2 = 16 + 64
    assert sums.tolist() == [np.sqrt(80.0), np.sqrt(80.0)]
    m = R.metrics_ref(stats[None, None], sums[None, None])
    assert m["hd"][0, 0] == m["hdp"][0, 0] == m["assd"][0, 0] == np.sqrt(80.0) and bool(m["scored"][0, 0])


def test_identical_masks_are_scored_with_zeros():
    rng = np.random.default_rng(3)
    a = rng.random((9, 12)) < 0.5
    stats, sums = R.plane_stats(a, a.copy())
    n = int(R.contour(a).sum())
    assert stats.tolist() == [[n, 0, 0, 0], [n, 0, 0, 0]] and sums.tolist() == [0.0, 0.0]
    m = R.metrics_ref(stats[None, None], sums[None, None])
    assert bool(m["scored"][0, 0]) and m["hd"][0, 0] == m["hdp"][0, 0] == m["assd"][0, 0] == 0.0


def test_full_plane_against_its_inset_rectangle():
    full = np.ones((8, 11), bool)
    inset = np.zeros_like(full)
    inset[1:-1, 1:-1] = True
    assert int(R.contour(full).sum()) == 2 * 8 + 2 * 11 - 4                       # a full plane: the image border
    stats, sums = R.plane_stats(full, inset)
    # inset contour -> border: every distance 1; border -> inset contour: 1, except the four corners (sqrt 2)
    n_in = 2 * 6 + 2 * 9 - 4
    assert stats[1].tolist() == [n_in, 1, 1, 1] and sums[1] == float(n_in)
    assert stats[0, 0] == 34 and stats[0, 1] == 2 and abs(sums[0] - (30 + 4 * np.sqrt(2.0))) < 1e-12
    one = np.ones((1, 1), bool)
    assert R.contour(one).tolist() == [[True]]                                     # a 1 x 1 on plane is its own contour


def test_empty_sides_fill_and_masks():
    a = np.zeros((4, 4), bool)
    b = a.copy()
    b[1:3, 1:3] = True
    for pred, targ, key in ((a, b, "missed"), (b, a, "spurious"), (a, a, "absent"), (b, b, "scored")):
        stats, sums = R.plane_stats(pred, targ)
        m = R.metrics_ref(stats[None, None], sums[None, None])
        assert [k for k in ("scored", "missed", "spurious", "absent") if m[k][0, 0]] == [key]
        if key != "scored":
            assert stats[:, 1:].tolist() == [[-1] * 3] * 2 and sums.tolist() == [0.0, 0.0]
            assert stats[:, 0].tolist() == [int(R.contour(pred).sum()), int(R.contour(targ).sum())]
            assert np.isnan(m["hd"][0, 0])


def test_predicates_on_planted_logits():
    x = np.array([0.0, -0.0, 1e-3, -1e-3, np.inf, -np.inf, np.nan, 1e-30], dtype=np.float32)
    assert R.pred_on(x).tolist() == [False, False, True, False, True, False, False, False]     # 1e-30: sigmoid rounds to 0.5 in fp32
    assert R.target_on(np.array([0.0, -0.0, 1.0, 0.5, np.nan])).tolist() == [False, False, True, True, True]


def test_report_counts_and_none():
    logits = np.full((2, 3, 4, 4), -5.0, np.float32)
    target = np.zeros((2, 3, 4, 4), np.float32)
    logits[:, 0, 1:3, 1:3] = 5.0
    target[:, 0, 1:3, 1:4] = 1.0                                                   # channel 0: scored in both frames
    target[0, 1, 0, 0] = 1.0                                                       # channel 1: missed once, absent once; channel 2: absent
    rep = R.report_ref([(logits, target)])
    assert rep["scored"] == [2, 0, 0] and rep["missed"] == [0, 1, 0] and rep["spurious"] == [0, 0, 0] and rep["absent"] == [0, 1, 2]
    assert rep["hd"][1] is None and rep["hd95"][2] is None and rep["assd"][1] is None
    assert rep["hd"][0] == 1.0 and rep["mean"][0] == 1.0
    assert R.report_ref([(np.full((1, 1, 2, 2), -1.0, np.float32), np.zeros((1, 1, 2, 2), np.float32))])["mean"] is None
