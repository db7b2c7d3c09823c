"""CPU: the fused SGD's C entry point (glf_sgd_step) is declared, exported and refuses bad arguments before it touches the
HIP runtime; glfusion_amd.optim.SGD has torch.optim.SGD's constructor checks and state-dict layout."""
import ctypes as C
import re

import pytest
import torch

from glfusion_amd import _lib
from glfusion_amd._lib import lib

GLF_ERR_BAD_SHAPE, GLF_ERR_NULL = -1, -5


def test_header_declares_and_library_exports_sgd_step():
    protos = _lib.parse_header()
    assert "glf_sgd_step" in protos
    restype, argtypes = protos["glf_sgd_step"]
    assert restype is C.c_int
    assert argtypes == [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int, C.c_int, C.c_void_p]
    dll = C.CDLL(_lib.LIB_PATH)
    assert hasattr(dll, "glf_sgd_step")
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                      # additive: the ABI version does not move
    # documented next to glf_adam_step
    text = open(_lib.HEADER).read()
    assert re.search(r"glf_adam_step\s*\([^;]*\);\s*/\*.*?\*/\s*int glf_sgd_step\s*\(", text, flags=re.S)


def test_sgd_step_argument_checks_need_no_gpu():
    buf = (C.c_int64 * 12)()                               # a host array: checked for null / alignment only, never read by the host
    tab = C.addressof(buf)
    assert tab % 8 == 0

    def call(table=tab, n_rows=1, lr=0.1, momentum=0.0, dampening=0.0, wd=0.0, nesterov=0, first=0):
        return lib.glf_sgd_step(table, n_rows, lr, momentum, dampening, wd, nesterov, first, None)

    assert call(table=None) == GLF_ERR_NULL and b"null table" in lib.glf_last_error()
    assert call(n_rows=0) == GLF_ERR_BAD_SHAPE and b"n_rows" in lib.glf_last_error()
    assert call(n_rows=-3) == GLF_ERR_BAD_SHAPE
    assert call(table=tab + 4) == GLF_ERR_BAD_SHAPE and b"aligned" in lib.glf_last_error()
    assert call(momentum=-0.5) == GLF_ERR_BAD_SHAPE and b"momentum" in lib.glf_last_error()
    assert call(nesterov=1, momentum=0.0) == GLF_ERR_BAD_SHAPE and b"nesterov" in lib.glf_last_error()
    assert call(nesterov=1, momentum=0.9, dampening=0.1) == GLF_ERR_BAD_SHAPE and b"nesterov" in lib.glf_last_error()
    # a null table wins over every other error
    assert call(table=None, n_rows=0, momentum=-1.0) == GLF_ERR_NULL


def test_sgd_raises_torchs_value_errors():
    from glfusion_amd.optim import SGD
    for kw in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.1), dict(lr=0.1, weight_decay=-1e-4), dict(lr=0.1, nesterov=True),
               dict(lr=0.1, nesterov=True, momentum=0.9, dampening=0.1)):
        with pytest.raises(ValueError) as ours:
            SGD([torch.nn.Parameter(torch.zeros(3))], **kw)
        with pytest.raises(ValueError) as theirs:
            torch.optim.SGD([torch.nn.Parameter(torch.zeros(3))], **kw)
        assert str(ours.value) == str(theirs.value), kw
    with pytest.raises(TypeError):
        SGD([torch.nn.Parameter(torch.zeros(3))])         # lr has no default


def test_sgd_state_dict_keys_are_torchs():
    from glfusion_amd.optim import SGD
    shapes = [(1,), (7,), (3, 5), (8, 4, 3, 3)]
    for kw in (dict(lr=0.1), dict(lr=0.05, momentum=0.9, weight_decay=1e-4), dict(lr=0.05, momentum=0.9, nesterov=True)):
        ours = SGD([torch.nn.Parameter(torch.zeros(*s)) for s in shapes], **kw)
        theirs = torch.optim.SGD([torch.nn.Parameter(torch.zeros(*s)) for s in shapes], **kw)
        a, b = ours.state_dict(), theirs.state_dict()
        assert set(a) == set(b) and a["state"] == b["state"] == {}
        assert len(a["param_groups"]) == len(b["param_groups"]) == 1
        assert a["param_groups"][0] == b["param_groups"][0]             # same keys, same values, same parameter indices
        assert ours.defaults == theirs.defaults
        theirs.load_state_dict(a)                                         # and each accepts the other's
        ours.load_state_dict(b)


def test_sgd_has_no_cpu_fallback():
    from glfusion_amd.optim import SGD
    p = [torch.nn.Parameter(torch.zeros(4))]
    o = SGD(p, lr=0.1)
    p[0].grad = torch.ones(4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        o.step()
    assert len(o.state) == 0
