"""CPU: the C entry point of the cross pseudo supervision loss (glf_cps_bce_sum) is declared directly after glf_overlap_counts,
exported, and refuses bad arguments before it touches the HIP runtime; ops.cps_bce_sum has no CPU fallback."""
import ctypes as C
import re

import pytest
import torch

from glfusion_amd import _lib
from glfusion_amd._lib import lib

GLF_ERR_BAD_SHAPE, GLF_ERR_NULL = -1, -5
P, F, L = C.c_void_p, C.c_float, C.c_int64
SIGNATURE = [P, P, P, P, P, P, F, P, L, P]      # a, b, loss_out, stats, da, db, grad_scale, grad_scale_dev, numel, stream


def test_header_declares_and_library_exports_cps_bce_sum():
    protos = _lib.parse_header()
    dll = C.CDLL(_lib.LIB_PATH)
    assert "glf_cps_bce_sum" in protos
    assert protos["glf_cps_bce_sum"][0] is C.c_int and protos["glf_cps_bce_sum"][1] == SIGNATURE
    assert hasattr(dll, "glf_cps_bce_sum")
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                      # additive: the ABI version does not move
    text = open(_lib.HEADER).read()
    # the declaration (with its comment) directly follows glf_overlap_counts
    assert re.search(r"int glf_overlap_counts\s*\([^;]*\);\s*/\*.*?\*/\s*int glf_cps_bce_sum\s*\(", text, flags=re.S)
    m = re.search(r"int glf_cps_bce_sum\s*\(([^;]*)\);", text, flags=re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ("const float* a, const float* b, double* loss_out, int64_t* stats, float* da, float* db, "
                                                       "float grad_scale, const float* grad_scale_dev, int64_t numel, glf_stream_t s")


def _err():
    return lib.glf_last_error()


def test_argument_checks_need_no_gpu():
    # host arrays: checked for null / aliasing only, never read by the host
    keep = [(C.c_float * 8)() for _ in range(4)] + [(C.c_double * 1)(), (C.c_int64 * 4)()]
    a, b, da, db, loss, stats = (C.addressof(x) for x in keep)

    def call(a=a, b=b, loss=loss, stats=stats, da=None, db=None, numel=8):
        return lib.glf_cps_bce_sum(a, b, loss, stats, da, db, 1.0, None, numel, None)

    for bad in (dict(a=None), dict(b=None), dict(loss=None)):
        assert call(**bad) == GLF_ERR_NULL and b"cps_bce_sum: null argument" in _err()
    # exactly one of da / db
    assert call(da=da) == GLF_ERR_NULL and b"cps_bce_sum: null argument" in _err()
    assert call(db=db) == GLF_ERR_NULL and b"cps_bce_sum: null argument" in _err()
    # a null pointer wins over every other error
    assert call(a=None, numel=0) == GLF_ERR_NULL
    assert call(b=None, da=a, db=a, numel=-3) == GLF_ERR_NULL
    assert call(da=da, numel=0) == GLF_ERR_NULL
    assert call(numel=0) == GLF_ERR_BAD_SHAPE and b"cps_bce_sum: numel must be > 0" in _err()
    assert call(numel=-1) == GLF_ERR_BAD_SHAPE and b"numel must be > 0" in _err()
    assert call(da=da, db=db, numel=0) == GLF_ERR_BAD_SHAPE and b"numel must be > 0" in _err()
    for bad in (dict(da=a, db=db), dict(da=da, db=b), dict(da=da, db=da)):
        assert call(**bad) == GLF_ERR_BAD_SHAPE and b"cps_bce_sum: outputs must not alias" in _err()
    assert call(stats=None, numel=0) == GLF_ERR_BAD_SHAPE            # stats may be NULL: not a null-argument error


def test_ops_cps_bce_sum_has_no_cpu_fallback():
    from glfusion_amd import ops
    a, b = torch.zeros(2, 5, 4, 4), torch.zeros(2, 5, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cps_bce_sum(a, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.cps_bce_sum(a.requires_grad_(True), b, torch.zeros(4, dtype=torch.int64))
