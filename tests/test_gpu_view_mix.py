"""GPU: the view-mix kernels (csrc/view_mix.hip; glf_view_mix_fwd / _dgrad / _wgrad) and ops.view_mix against a float64 torch
evaluation of  y_v[r][o] = b_v[o] + sum_u sum_i W_v[o][u c + i] x_u[r][i]  on the CPU.

Gates, element-wise, u = 2^-24:
  forward, dgrad   |got - want| <= 2 (V c + 1) u (|b| + sum |W| |x|)     the fp32 dot-product bound for V c + 1 terms, factor 2
  wgrad            |got - want| <= (rows + 2) u sum_r |dy x|             holds for any summation order in fp32
Shapes: R = the wgrad row run, G = 4 rows per thread at c = 1 and c = 5: rows around G, around one workgroup (1024 = 256 threads x 4
rows), around R and past 2 R."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
VC_CASES = [(1, 1), (2, 1), (3, 1), (3, 5), (5, 5), (5, 8), (8, 5)]


def _ops():
    from glfusion_amd import ops
    return ops


def R():
    return _ops().VIEW_MIX_WGRAD_ROWS


def row_counts():
    r = R()
    return [1, 3, 4, 5, 1023, 1025, r - 1, r, r + 1, 2 * r + 3]


def rnd(shape, seed):
    return 2.0 * torch.rand(shape, generator=torch.Generator().manual_seed(seed)) - 1.0          # [-1, 1]


def table(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def call(name, *args):
    from glfusion_amd._lib import check, lib
    check(getattr(lib, "glf_" + name)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args], None), name)
    torch.cuda.synchronize()


def case(v, c, rows, seed):
    vc = v * c
    xs = [rnd((rows, c), seed + u) for u in range(v)]
    dys = [rnd((rows, c), seed + 50 + u) for u in range(v)]
    ws = [rnd((c, vc, 1, 1), seed + 100 + u) for u in range(v)]
    bs = [rnd((c,), seed + 150 + u) for u in range(v)]
    return xs, dys, ws, bs


def want_all(xs, dys, ws, bs):
    """float64: (y, |.| bound of y), (dx, bound), (dW, bound), (db, bound), each over the concatenated [rows][V c] / [V c][V c] forms."""
    X, D = torch.cat(xs, dim=1).double(), torch.cat(dys, dim=1).double()
    Wm, bm = _ops().view_mix_stack(ws, bs)
    Wm, bm = Wm.double(), bm.double()
    return ((X @ Wm.t() + bm, X.abs() @ Wm.abs().t() + bm.abs()), (D @ Wm, D.abs() @ Wm.abs()),
            (D.t() @ X, D.abs().t() @ X.abs()), (D.sum(dim=0), D.abs().sum(dim=0)))


def within(got, want, mag, factor, what):
    got = got.detach()
    err = (got.double().cpu() - want).abs()
    ok = bool((err <= factor * U * mag).all()) and bool(torch.isfinite(got).all())          # no NaN of the pre-fill survives
    worst = float((err / (factor * U * mag).clamp_min(1e-300)).max())
    print(f"{what}: worst element at {worst:.3f} of its bound")
    return ok


def run_kernels(xs, dys, ws, bs):
    v, c, rows = len(xs), xs[0].shape[1], xs[0].shape[0]
    vc = v * c
    from glfusion_amd._lib import lib
    Wm, bm = _ops().view_mix_stack(ws, bs)
    Wm, bm = Wm.to(DEV).contiguous(), bm.to(DEV).contiguous()
    xd, dyd = [t.to(DEV) for t in xs], [t.to(DEV) for t in dys]
    nan = float("nan")
    ys = [torch.full((rows, c), nan, device=DEV) for _ in range(v)]
    dxs = [torch.full((rows, c), nan, device=DEV) for _ in range(v)]
    call("view_mix_fwd", table(xd), Wm, bm, table(ys), rows, v, c)
    call("view_mix_dgrad", table(dyd), Wm, table(dxs), rows, v, c)
    need = int(lib.glf_view_mix_wgrad_workspace(rows, v, c))
    assert need == -(-rows // R()) * vc * (vc + 1) * 4
    out = []
    for _ in range(2):
        dw, db = torch.full((vc, vc), nan, device=DEV), torch.full((vc,), nan, device=DEV)
        ws_ = torch.full((need // 4,), nan, device=DEV)                                      # the workspace needs no clearing
        call("view_mix_wgrad", table(xd), table(dyd), dw, db, ws_, need, rows, v, c)
        out.append((dw.cpu(), db.cpu()))
    return torch.cat(ys, dim=1), torch.cat(dxs, dim=1), out


@pytest.mark.parametrize("v,c", VC_CASES)
def test_view_mix_kernels_against_float64(v, c):
    vc = v * c
    for rows in row_counts():
        xs, dys, ws, bs = case(v, c, rows, 1000 * v + 10 * c)
        (wy, my), (wdx, mdx), (wdw, mdw), (wdb, mdb) = want_all(xs, dys, ws, bs)
        y, dx, ((dw, db), (dw2, db2)) = run_kernels(xs, dys, ws, bs)
        tag = f"V {v} c {c} rows {rows}"
        assert within(y, wy, my, 2 * (vc + 1), tag + " forward"), tag
        assert within(dx, wdx, mdx, 2 * (vc + 1), tag + " dgrad"), tag
        assert within(dw, wdw, mdw, rows + 2, tag + " dW"), tag
        assert within(db, wdb, mdb, rows + 2, tag + " db"), tag
        assert torch.equal(dw, dw2) and torch.equal(db, db2), tag                           # no atomics: the same bits again


def test_view_mix_forward_without_bias_and_wgrad_without_db():
    v, c, rows = 3, 5, 37
    xs, dys, ws, bs = case(v, c, rows, 7)
    (wy, my), _, (wdw, mdw), _ = want_all(xs, dys, ws, [torch.zeros(c) for _ in range(v)])
    from glfusion_amd._lib import lib
    Wm = _ops().view_mix_stack(ws, bs)[0].to(DEV).contiguous()
    xd, dyd = [t.to(DEV) for t in xs], [t.to(DEV) for t in dys]
    ys = [torch.full((rows, c), float("nan"), device=DEV) for _ in range(v)]
    call("view_mix_fwd", table(xd), Wm, None, table(ys), rows, v, c)
    assert within(torch.cat(ys, dim=1), wy, my, 2 * (v * c + 1), "no bias")
    need = int(lib.glf_view_mix_wgrad_workspace(rows, v, c))
    dw, part = torch.full((v * c, v * c), float("nan"), device=DEV), torch.empty(need // 4, device=DEV)
    call("view_mix_wgrad", table(xd), table(dyd), dw, None, part, need, rows, v, c)
    assert within(dw, wdw, mdw, rows + 2, "dW without db")


@pytest.mark.parametrize("v,c", [(5, 9), (9, 1), (6, 7)])
def test_view_mix_refuses_what_is_past_its_limits(v, c):
    ops = _ops()
    rows = 8
    bufs = [torch.zeros(rows, c, device=DEV) for _ in range(v)]
    outs = [torch.zeros(rows, c, device=DEV) for _ in range(v)]
    w, b = torch.zeros(v * c, v * c, device=DEV), torch.zeros(v * c, device=DEV)
    limit = "c <= 8, V <= 8, V \\* c <= 40"
    with pytest.raises(RuntimeError, match=limit):
        call("view_mix_fwd", table(bufs), w, b, table(outs), rows, v, c)
    with pytest.raises(RuntimeError, match=limit):
        call("view_mix_dgrad", table(bufs), w, table(outs), rows, v, c)
    with pytest.raises(RuntimeError, match=limit):
        call("view_mix_wgrad", table(bufs), table(outs), w, b, torch.zeros(1 << 16, device=DEV), 4 << 16, rows, v, c)
    ws = [torch.zeros(c, v * c, 1, 1, device=DEV) for _ in range(v)]
    with pytest.raises(RuntimeError, match=limit):
        ops.view_mix(bufs, ws, [torch.zeros(c, device=DEV) for _ in range(v)])


def test_view_mix_refuses_bad_arguments():
    from glfusion_amd._lib import lib
    ops = _ops()
    v, c, rows = 3, 5, R() + 1
    xs, dys, ws, bs = case(v, c, rows, 3)
    xd, dyd = [t.to(DEV) for t in xs], [t.to(DEV) for t in dys]
    dw, db = torch.empty(15, 15, device=DEV), torch.empty(15, device=DEV)
    need = int(lib.glf_view_mix_wgrad_workspace(rows, v, c))
    part = torch.empty(need // 4, device=DEV)
    call("view_mix_wgrad", table(xd), table(dyd), dw, db, part, need, rows, v, c)
    with pytest.raises(RuntimeError, match="workspace"):
        call("view_mix_wgrad", table(xd), table(dyd), dw, db, part, need - 1, rows, v, c)       # one byte short
    with pytest.raises(RuntimeError, match="rows, v and c must be positive"):
        call("view_mix_fwd", table(xd), dw, db, table(dyd), 0, v, c)
    with pytest.raises(RuntimeError, match="null argument"):
        call("view_mix_fwd", table(xd), None, db, table(dyd), rows, v, c)
    with pytest.raises(RuntimeError, match="non-null and 16-byte aligned"):
        call("view_mix_fwd", (C.c_void_p * 3)(xd[0].data_ptr(), None, xd[2].data_ptr()), dw, db, table(dyd), rows, v, c)
    with pytest.raises(RuntimeError, match="non-null and 16-byte aligned"):
        call("view_mix_fwd", (C.c_void_p * 3)(xd[0].data_ptr(), xd[1].data_ptr() + 4, xd[2].data_ptr()), dw, db, table(dyd), rows, v, c)
    # the autograd node: fp32, contiguous, one shape
    wd, bd = [t.to(DEV) for t in ws], [t.to(DEV) for t in bs]
    with pytest.raises(RuntimeError, match="float32"):
        ops.view_mix([xd[0].bfloat16(), xd[1], xd[2]], wd, bd)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.view_mix([torch.zeros(5, rows, device=DEV).t(), xd[1], xd[2]], wd, bd)
    with pytest.raises(RuntimeError, match="shape"):
        ops.view_mix([xd[0][:7], xd[1], xd[2]], wd, bd)


def _autograd_case(requires_input_grad):
    ops = _ops()
    v, c, rows = 3, 5, 37
    xs, dys, ws, bs = case(v, c, rows, 11)
    xd = [t.to(DEV).view(1, rows, 1, c).requires_grad_(requires_input_grad) for t in xs]        # channels-last [N,h,w,c]
    wd = [torch.nn.Parameter(t.to(DEV)) for t in ws]
    bd = [torch.nn.Parameter(t.to(DEV)) for t in bs]
    ys = ops.view_mix(xd, wd, bd)
    assert len(ys) == v and all(tuple(y.shape) == (1, rows, 1, c) and y.is_contiguous() for y in ys)
    torch.autograd.backward(ys, [t.to(DEV).view(1, rows, 1, c) for t in dys])
    torch.cuda.synchronize()
    return (xs, dys, ws, bs), xd, wd, bd, ys


def test_ops_view_mix_gradients_against_float64():
    (xs, dys, ws, bs), xd, wd, bd, ys = _autograd_case(True)
    v, c, rows = 3, 5, 37
    (wy, my), (wdx, mdx), (wdw, mdw), (wdb, mdb) = want_all(xs, dys, ws, bs)
    f = 2 * (v * c + 1)
    assert within(torch.cat([y.detach().reshape(rows, c) for y in ys], dim=1), wy, my, f, "ops forward")
    assert within(torch.cat([t.grad.reshape(rows, c) for t in xd], dim=1), wdx, mdx, f, "ops input gradients")
    assert all(tuple(p.grad.shape) == (c, v * c, 1, 1) for p in wd) and all(tuple(p.grad.shape) == (c,) for p in bd)
    assert within(torch.cat([p.grad.reshape(c, v * c) for p in wd], dim=0), wdw, mdw, rows + 2, "ops weight gradients")
    assert within(torch.cat([p.grad for p in bd], dim=0), wdb, mdb, rows + 2, "ops bias gradients")
    # the stacked operand follows the parameters: after an in-place update the next call mixes with the new values
    with torch.no_grad():
        for p in wd + bd:
            p.mul_(0.5)
    ys2 = _ops().view_mix([t.detach() for t in xd], wd, bd)
    torch.cuda.synchronize()
    assert within(torch.cat([y.reshape(rows, c) for y in ys2], dim=1), 0.5 * wy, 0.5 * my, f, "after a weight update")


def test_ops_view_mix_returns_no_input_gradient_for_data(monkeypatch):
    """Inputs that do not require grad (early_fusion's images): no gradient comes back for them, and the dgrad kernel is not launched."""
    from glfusion_amd._lib import lib
    launched = []
    real = lib.load().glf_view_mix_dgrad
    monkeypatch.setattr(lib.load(), "glf_view_mix_dgrad", lambda *a: launched.append(1) or real(*a))
    (xs, dys, ws, bs), xd, wd, bd, ys = _autograd_case(False)
    assert not launched and all(t.grad is None for t in xd)
    _, _, (wdw, mdw), _ = want_all(xs, dys, ws, bs)
    assert within(torch.cat([p.grad.reshape(5, 15) for p in wd], dim=0), wdw, mdw, 37 + 2, "weight gradients, data inputs")
    _autograd_case(True)
    assert launched == [1]
