"""CPU: glf_contour_distances is declared where the header's readers expect it, exported, and refuses bad arguments before it touches
the HIP runtime, in the documented order; the Python surface has no CPU fallback."""
import ctypes as C
import re

import pytest
import torch

from glfusion_amd import _lib, data
from glfusion_amd._lib import lib

GLF_ERR_BAD_SHAPE, GLF_ERR_UNSUPPORTED, GLF_ERR_NULL = -1, -2, -5
P, I = C.c_void_p, C.c_int


def _err():
    return lib.glf_last_error()


def test_header_declares_and_library_exports_contour_distances():
    protos = _lib.parse_header()
    assert "glf_contour_distances" in protos
    restype, argtypes = protos["glf_contour_distances"]
    assert restype is C.c_int and argtypes == [P, P, P, P, I, I, I, I, I, P]
    dll = C.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, "glf_contour_distances")
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                                           # additive: the ABI version does not move
    text = open(_lib.HEADER).read()
    assert text.index("int glf_prepare_batch(") < text.index("int glf_contour_distances(") < text.index("int glf_zero(")
    # behind a comment block of its own, which states the bound
    assert re.search(r"glf_prepare_batch\s*\([^;]*\);\s*/\*.*?\*/\s*(#define GLF_CONTOUR_MAX_DIM \d+\s*)?int glf_contour_distances\s*\(", text, flags=re.S)
    bound = int(re.search(r"#define GLF_CONTOUR_MAX_DIM (\d+)", text).group(1))
    assert 224 <= bound <= 1024


def test_error_codes_are_the_headers():
    text = open(_lib.HEADER).read()
    for name, value in (("GLF_ERR_BAD_SHAPE", GLF_ERR_BAD_SHAPE), ("GLF_ERR_UNSUPPORTED", GLF_ERR_UNSUPPORTED), ("GLF_ERR_NULL", GLF_ERR_NULL)):
        assert re.search(rf"{name}\s*=\s*{value}\b", text), name


def test_argument_checks_need_no_gpu():
    buf = (C.c_int64 * 16)()                     # stand-ins for the device arrays: checked for null only, never read or written
    dev = C.addressof(buf)
    bound = int(re.search(r"#define GLF_CONTOUR_MAX_DIM (\d+)", open(_lib.HEADER).read()).group(1))

    def call(logits=dev, target=dev + 32, stats=dev + 64, sums=dev + 96, n=1, c=5, h=112, w=112, pct=95):
        return lib.glf_contour_distances(logits, target, stats, sums, n, c, h, w, pct, None)

    for name in ("logits", "target", "stats", "sums"):
        assert call(**{name: None}) == GLF_ERR_NULL and b"contour_distances" in _err(), name
        # a null pointer wins over every other error
        assert call(**{name: None}, n=0, pct=101, h=bound + 1) == GLF_ERR_NULL and b"contour_distances" in _err(), name
    for bad in (dict(n=0), dict(c=0), dict(h=0), dict(w=0), dict(n=-1), dict(w=-7), dict(pct=-1), dict(pct=101)):
        assert call(**bad) == GLF_ERR_BAD_SHAPE and b"contour_distances" in _err(), bad
        too_wide = {"w" if "h" in bad else "h": bound + 1}
        assert call(**bad, **({} if "w" in bad else too_wide)) == GLF_ERR_BAD_SHAPE, bad         # shape before support
    assert call(n=0, w=bound + 1) == GLF_ERR_BAD_SHAPE and call(pct=200, w=5000) == GLF_ERR_BAD_SHAPE
    for bad in (dict(h=bound + 1), dict(w=bound + 1), dict(h=4096, w=4096)):
        assert call(**bad) == GLF_ERR_UNSUPPORTED and b"contour_distances" in _err() and str(bound).encode() in _err(), bad


def test_python_surface_has_no_cpu_fallback():
    x = torch.zeros(2, 5, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.contour_stats(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        data.ContourAccumulator(5, "cpu").add(x, x)


def test_contour_metrics_arithmetic_on_host_tensors():
    # contour_metrics is torch arithmetic: the same numbers wherever the tensors live
    stats = torch.tensor([[[[3, 25, 4, 9], [2, 16, 1, 16]], [[0, -1, -1, -1], [4, -1, -1, -1]],
                           [[5, -1, -1, -1], [0, -1, -1, -1]], [[0, -1, -1, -1], [0, -1, -1, -1]]]], dtype=torch.int64)
    sums = torch.tensor([[[6.0, 5.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0]]], dtype=torch.float64)
    m = data.contour_metrics(stats, sums, percentile=95)
    assert [[k for k in ("scored", "missed", "spurious", "absent") if bool(m[k][0, c])] for c in range(4)] == \
        [["scored"], ["missed"], ["spurious"], ["absent"]]
    # direction 0: 95 * 2 = 190 -> frac 0.9 between 2 and 3; direction 1: 95 * 1 -> frac 0.95 between 1 and 4
    assert float(m["hd"][0, 0]) == 5.0 and abs(float(m["hdp"][0, 0]) - 3.85) < 1e-12 and float(m["assd"][0, 0]) == 11.0 / 5.0
    with pytest.raises(ValueError):
        data.contour_metrics(stats, sums, percentile=101)
    with pytest.raises(RuntimeError):
        data.contour_metrics(stats.float(), sums)
    rep = data.ContourAccumulator.report_from_rows([[2.0, 3.0, 1.0, 2.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0, 3.0, 0.0, 1.0]])
    assert rep == {"hd": [1.0, None], "hd95": [1.5, None], "assd": [0.5, None], "scored": [2, 0], "missed": [0, 3], "spurious": [1, 0],
                   "absent": [0, 1], "mean": (1.0, 1.5, 0.5)}
    assert data.ContourAccumulator.report_from_rows([[0.0] * 7])["mean"] is None
