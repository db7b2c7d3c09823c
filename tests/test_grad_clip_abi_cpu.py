"""CPU: the C entry points of the fused global-norm gradient clipping (glf_grad_sumsq, glf_grad_clip_coef, glf_adam_step_clipped,
glf_sgd_step_clipped, glf_grad_scale) are declared, exported and refuse bad arguments before they touch the HIP runtime;
set_grad_clip leaves the optimizers' defaults and state dicts torch's."""
import ctypes as C
import math
import re

import pytest
import torch

from glfusion_amd import _lib
from glfusion_amd._lib import lib

GLF_ERR_BAD_SHAPE, GLF_ERR_NULL = -1, -5
P, I, D, L = C.c_void_p, C.c_int, C.c_double, C.c_int64
SIGNATURES = {
    "glf_grad_sumsq": [P, I, P, P],
    "glf_grad_clip_coef": [P, I, D, P, P, P],
    "glf_adam_step_clipped": [P, I, D, D, D, D, D, L, P, P],
    "glf_sgd_step_clipped": [P, I, D, D, D, D, I, I, P, P],
    "glf_grad_scale": [P, I, P, P],
}


def test_header_declares_and_library_exports_the_clip_functions():
    protos = _lib.parse_header()
    dll = C.CDLL(_lib.LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        assert name in protos, name
        assert protos[name][0] is C.c_int and protos[name][1] == argtypes, name
        assert hasattr(dll, name), name
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                      # additive: the ABI version does not move
    text = open(_lib.HEADER).read()
    # glf_sgd_step still directly follows glf_adam_step and its comment (tests/test_sgd_abi_cpu.py); the new ones come after it
    assert re.search(r"glf_adam_step\s*\([^;]*\);\s*/\*.*?\*/\s*int glf_sgd_step\s*\(", text, flags=re.S)
    assert all(text.index("int glf_sgd_step(") < text.index(f"int {name}(") for name in SIGNATURES)


def _host_arrays():
    # host arrays: checked for null / alignment only, never read by the host
    buf, part, rec, cnt = (C.c_int64 * 12)(), (C.c_double * 4)(), (C.c_float * 4)(), (C.c_int64 * 2)()
    keep = (buf, part, rec, cnt)
    tab, part, rec, cnt = (C.addressof(x) for x in keep)
    assert tab % 8 == 0 and part % 8 == 0
    return keep, tab, part, rec, cnt


def _err():
    return lib.glf_last_error()


def test_sumsq_and_scale_argument_checks_need_no_gpu():
    keep, tab, part, rec, cnt = _host_arrays()
    assert lib.glf_grad_sumsq(None, 1, part, None) == GLF_ERR_NULL and b"null table" in _err()
    assert lib.glf_grad_sumsq(tab, 1, None, None) == GLF_ERR_NULL and b"null partials" in _err()
    assert lib.glf_grad_sumsq(None, 0, part + 4, None) == GLF_ERR_NULL           # a null pointer wins over every other error
    assert lib.glf_grad_sumsq(tab, 0, part, None) == GLF_ERR_BAD_SHAPE and b"n_rows" in _err()
    assert lib.glf_grad_sumsq(tab, -2, part, None) == GLF_ERR_BAD_SHAPE
    assert lib.glf_grad_sumsq(tab + 4, 1, part, None) == GLF_ERR_BAD_SHAPE and b"table must be 8-byte aligned" in _err()
    assert lib.glf_grad_sumsq(tab, 1, part + 4, None) == GLF_ERR_BAD_SHAPE and b"partials must be 8-byte aligned" in _err()

    assert lib.glf_grad_scale(None, 1, rec, None) == GLF_ERR_NULL and b"null table" in _err()
    assert lib.glf_grad_scale(tab, 1, None, None) == GLF_ERR_NULL and b"null record" in _err()
    assert lib.glf_grad_scale(None, 0, None, None) == GLF_ERR_NULL
    assert lib.glf_grad_scale(tab, 0, rec, None) == GLF_ERR_BAD_SHAPE and b"n_rows" in _err()
    assert lib.glf_grad_scale(tab + 4, 1, rec, None) == GLF_ERR_BAD_SHAPE and b"aligned" in _err()


def test_clip_coef_argument_checks_need_no_gpu():
    keep, tab, part, rec, cnt = _host_arrays()

    def call(partials=part, n=1, max_norm=1.0, record=rec, skipped=cnt):
        return lib.glf_grad_clip_coef(partials, n, max_norm, record, skipped, None)

    assert call(partials=None) == GLF_ERR_NULL and b"null partials" in _err()
    assert call(record=None) == GLF_ERR_NULL and b"null record" in _err()
    assert call(skipped=None) == GLF_ERR_NULL and b"null skipped" in _err()
    assert call(partials=None, n=0, max_norm=-1.0) == GLF_ERR_NULL                # a null pointer wins over every other error
    assert call(n=0) == GLF_ERR_BAD_SHAPE and b"n must be > 0" in _err()
    assert call(n=-1) == GLF_ERR_BAD_SHAPE
    assert call(partials=part + 4) == GLF_ERR_BAD_SHAPE and b"partials must be 8-byte aligned" in _err()
    assert call(max_norm=-1.0) == GLF_ERR_BAD_SHAPE and b"max_norm" in _err()
    assert call(max_norm=math.nan) == GLF_ERR_BAD_SHAPE and b"max_norm" in _err()
    assert call(max_norm=-math.inf) == GLF_ERR_BAD_SHAPE and b"max_norm" in _err()


def test_clipped_step_argument_checks_need_no_gpu():
    keep, tab, part, rec, cnt = _host_arrays()

    def sgd(table=tab, n_rows=1, lr=0.1, momentum=0.0, dampening=0.0, wd=0.0, nesterov=0, first=0, record=rec):
        return lib.glf_sgd_step_clipped(table, n_rows, lr, momentum, dampening, wd, nesterov, first, record, None)

    assert sgd(table=None) == GLF_ERR_NULL and b"null table" in _err()
    assert sgd(record=None) == GLF_ERR_NULL and b"null record" in _err()
    assert sgd(n_rows=0) == GLF_ERR_BAD_SHAPE and b"n_rows" in _err()
    assert sgd(table=tab + 4) == GLF_ERR_BAD_SHAPE and b"aligned" in _err()
    assert sgd(momentum=-0.5) == GLF_ERR_BAD_SHAPE and b"momentum" in _err()
    assert sgd(nesterov=1, momentum=0.0) == GLF_ERR_BAD_SHAPE and b"nesterov" in _err()
    assert sgd(nesterov=1, momentum=0.9, dampening=0.1) == GLF_ERR_BAD_SHAPE and b"nesterov" in _err()
    assert b"sgd_step_clipped" in _err()
    assert sgd(record=None, n_rows=0, momentum=-1.0) == GLF_ERR_NULL              # a null pointer wins over every other error

    def adam(table=tab, n_rows=1, step=1, record=rec):
        return lib.glf_adam_step_clipped(table, n_rows, 1e-3, 0.9, 0.999, 1e-8, 0.0, step, record, None)

    assert adam(table=None) == GLF_ERR_NULL and b"null table" in _err()
    assert adam(record=None) == GLF_ERR_NULL and b"null record" in _err()
    assert adam(n_rows=0) == GLF_ERR_BAD_SHAPE and b"n_rows" in _err()
    assert adam(table=tab + 4) == GLF_ERR_BAD_SHAPE and b"aligned" in _err()
    assert adam(step=0) == GLF_ERR_BAD_SHAPE and b"step counts from 1" in _err()
    assert adam(table=None, n_rows=0, step=0) == GLF_ERR_NULL


SHAPES = [(1,), (7,), (3, 5), (8, 4, 3, 3)]


@pytest.mark.parametrize("bad", [-1.0, -1e-30, math.nan, -math.inf])
def test_set_grad_clip_refuses_bad_max_norm(bad):
    from glfusion_amd.optim import SGD, Adam, clip_grad_norm_
    for opt in (Adam([torch.nn.Parameter(torch.zeros(3))]), SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)):
        with pytest.raises(ValueError, match="max_norm"):
            opt.set_grad_clip(bad)
    with pytest.raises(ValueError, match="max_norm"):
        clip_grad_norm_([torch.nn.Parameter(torch.zeros(3))], bad)


def test_set_grad_clip_accepts_zero_inf_and_none():
    from glfusion_amd.optim import SGD
    opt = SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, momentum=0.9)
    assert opt.grad_norm is None and opt.skipped_steps is None
    for ok in (0.0, 1, 2.5, math.inf, None):
        opt.set_grad_clip(ok)


def test_set_grad_clip_leaves_defaults_and_state_dict_torchs():
    from glfusion_amd.optim import SGD, Adam
    cases = [(Adam, torch.optim.Adam, dict(lr=3e-4, weight_decay=1e-5)), (SGD, torch.optim.SGD, dict(lr=0.1)),
             (SGD, torch.optim.SGD, dict(lr=0.05, momentum=0.9, weight_decay=1e-4))]
    for ours_cls, theirs_cls, kw in cases:
        ours = ours_cls([torch.nn.Parameter(torch.zeros(*s)) for s in SHAPES], **kw)
        plain = ours_cls([torch.nn.Parameter(torch.zeros(*s)) for s in SHAPES], **kw)
        theirs = theirs_cls([torch.nn.Parameter(torch.zeros(*s)) for s in SHAPES], **kw)
        ours.set_grad_clip(1.0)
        a, b = ours.state_dict(), theirs.state_dict()
        assert a == plain.state_dict() and ours.defaults == plain.defaults
        assert set(a) == set(b) and a["state"] == b["state"] == {}
        if ours_cls is SGD:
            assert a["param_groups"] == b["param_groups"] and ours.defaults == theirs.defaults
        else:
            # Adam carries the keys of the reference's torch (1.8.1): each of them with torch's value, none added
            assert all(b["param_groups"][0][k] == v for k, v in a["param_groups"][0].items())
            assert all(theirs.defaults[k] == v for k, v in ours.defaults.items())
        assert not any("clip" in k or "max_norm" in k for g in ours.param_groups for k in g)
        theirs.load_state_dict(a)                                         # and each accepts the other's
        ours.load_state_dict(b)


def test_clipped_step_has_no_cpu_fallback():
    from glfusion_amd.optim import SGD, Adam, clip_grad_norm_, grad_norm
    for make in (lambda p: Adam(p), lambda p: SGD(p, lr=0.1, momentum=0.9)):
        p = [torch.nn.Parameter(torch.zeros(4))]
        o = make(p)
        o.set_grad_clip(1.0)
        p[0].grad = torch.ones(4)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            o.step()
        assert len(o.state) == 0
    for fn in (grad_norm, lambda ps: clip_grad_norm_(ps, 1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(p)
