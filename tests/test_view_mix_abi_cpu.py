"""CPU: the view-mix entry points (glf_view_mix_fwd / _dgrad / _wgrad_workspace / _wgrad, csrc/view_mix.hip) are declared with the
documented signatures, bound by _lib.parse_header and exported; the workspace query (host-only) counts one block of V c (V c + 1)
partial sums per run of rows; ops.view_mix_stack is the index permutation the kernels assume."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from glfusion_amd import _lib
from glfusion_amd._lib import lib

P, I, L, Z = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
SIGNATURES = {
    "glf_view_mix_fwd": (C.c_int, [P, P, P, P, L, I, I, P]),                       # xs, w, bias, ys, rows, v, c, stream
    "glf_view_mix_dgrad": (C.c_int, [P, P, P, L, I, I, P]),                        # dys, w, dxs, rows, v, c, stream
    "glf_view_mix_wgrad_workspace": (Z, [L, I, I]),                                # rows, v, c
    "glf_view_mix_wgrad": (C.c_int, [P, P, P, P, P, Z, L, I, I, P]),               # xs, dys, dw, db, workspace, bytes, rows, v, c, stream
}


def test_header_declares_and_library_exports_the_view_mix():
    protos = _lib.parse_header()
    dll = C.CDLL(_lib.LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        assert name in protos, name
        assert protos[name][0] is restype and protos[name][1] == argtypes, (name, protos[name])
        assert hasattr(dll, name), name
        assert getattr(lib, name).argtypes == argtypes                              # bound on the loaded library
    dll.glf_abi_version.restype = C.c_int
    assert dll.glf_abi_version() == 7                      # additive: the ABI version does not move


def test_workspace_query_counts_one_block_of_sums_per_row_run():
    from glfusion_amd import ops
    q, R = lib.glf_view_mix_wgrad_workspace, ops.VIEW_MIX_WGRAD_ROWS
    assert R == 1024
    for v, c in ((1, 1), (3, 1), (3, 5), (5, 5), (5, 8), (8, 5)):
        sums = v * c * (v * c + 1)
        assert q(1, v, c) == q(R, v, c) == 4 * sums and q(R + 1, v, c) == 8 * sums and q(2 * R + 3, v, c) == 12 * sums
    # outside the limits (c <= 8, V <= 8, V c <= 40) and for empty extents there is nothing to size
    for rows, v, c in ((0, 3, 5), (-1, 3, 5), (10, 0, 5), (10, 3, 0), (10, 5, 9), (10, 9, 1), (10, 6, 7)):
        assert q(rows, v, c) == 0
    assert (ops.VIEW_MIX_MAX_V, ops.VIEW_MIX_MAX_C, ops.VIEW_MIX_MAX_VC) == (8, 8, 40)


@pytest.mark.parametrize("v,c", [(1, 1), (2, 1), (3, 1), (3, 5), (5, 5), (5, 8), (8, 5)])
def test_stacking_is_a_pure_index_permutation(v, c):
    """Wm[v c + o][u c + i] = W_v[o][u c + i], bm[v c + o] = b_v[o]: the rows of the stacked matrix ARE the rows of the V weights, so a
    1x1 convolution with row block v of Wm over torch.cat(xs, dim=1) is bit for bit fc[v] over it, in float64."""
    from glfusion_amd import ops
    g = torch.Generator().manual_seed(100 * v + c)
    ws = [torch.randn(c, v * c, 1, 1, dtype=torch.float64, generator=g) for _ in range(v)]
    bs = [torch.randn(c, dtype=torch.float64, generator=g) for _ in range(v)]
    xs = [torch.randn(2, c, 3, 5, dtype=torch.float64, generator=g) for _ in range(v)]
    Wm, bm = ops.view_mix_stack(ws, bs)
    assert tuple(Wm.shape) == (v * c, v * c) and tuple(bm.shape) == (v * c,) and Wm.dtype == torch.float64
    for k in range(v):
        for o in range(c):
            assert torch.equal(bm[k * c + o], bs[k][o])
            for u in range(v):
                assert torch.equal(Wm[k * c + o, u * c:(u + 1) * c], ws[k][o, u * c:(u + 1) * c, 0, 0])
    cat = torch.cat(xs, dim=1)
    for k in range(v):
        assert torch.equal(F.conv2d(cat, Wm[k * c:(k + 1) * c].view(c, v * c, 1, 1), bm[k * c:(k + 1) * c]), F.conv2d(cat, ws[k], bs[k]))


def test_stacking_refuses_mismatched_operands():
    from glfusion_amd import ops
    w = [torch.zeros(5, 15, 1, 1) for _ in range(3)]
    b = [torch.zeros(5) for _ in range(3)]
    with pytest.raises(RuntimeError, match="view_mix"):
        ops.view_mix_stack(w[:2], b[:2])                    # two weights of a three-view mix
    with pytest.raises(RuntimeError, match="view_mix"):
        ops.view_mix_stack(w, b[:2] + [torch.zeros(4)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.view_mix([torch.zeros(2, 4, 4, 5) for _ in range(3)], w, b)
