"""The ASPP head's input gradient as ONE segmented region-mode launch (glf_gemm_params.nseg, ops.ASPP_DGRAD_ONE) against the
three launches it replaces: the stacked centre contraction plus one accumulating launch per branch that keeps off-centre taps.

Yardstick (the one test_gpu_aspp_centre.py uses): against a float64 result on the CPU computed from the same operand values,
the one-launch route's relative L2 error must be <= 1.5 x the three-launch route's error + 1e-7.  Both routes sum the same
products; the one launch does it under ONE weight scale (the maximum of the stacked image, at most the largest branch maximum:
up to one split bit lost for the other branches) and in one chain instead of three rounded partial results.  A wrong segment
offset, column block or region misses the bound by orders of magnitude.  Both errors are printed."""
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_aspp_centre as base                              # the shared float64 oracle, the train-step runner and its yardstick

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (n, h, w, Cin, Cout, rates).  d: 7 x 7 bands on a non-square map, rate 7's interior is centre-only.  a: the model's band
# structure (ragged tiles, rate 24's interior empty, rate 36 centre-only).  b: one rate >= both extents of a non-square map.
SHAPES = {"d": (2, 9, 12, 64, 32, (2, 4, 7)), "a": (3, 28, 28, 64, 32, (12, 24, 36)), "b": (2, 12, 10, 64, 32, (3, 6, 12))}
base.SHAPES.setdefault("dgrad_one_d", SHAPES["d"])
MODULE_SHAPES = {"d": "dgrad_one_d", "a": "a", "b": "b"}         # keys of the shared oracle


def _rel(a, ref):
    return float((a.detach().cpu().double() - ref).norm()) / max(float(ref.norm()), 1e-300)


_OPERANDS = {}


def _operands(shape):
    """G [rows][k Cout], the four weights and the float64 input gradient of the four convolutions, once per shape."""
    if shape not in _OPERANDS:
        n, h, w, cin, cout, rates = SHAPES[shape]
        k = 1 + len(rates)
        g = torch.Generator().manual_seed(11)
        G = torch.randn(n, h, w, k * cout, generator=g)
        ws = [torch.randn(cout, cin, 1, 1, generator=g) * 0.7] + [torch.randn(cout, cin, 3, 3, generator=g) * (0.3 + 0.4 * i) for i in range(len(rates))]
        x = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
        tot = 0.0
        for i, wt in enumerate(ws):
            d = 1 if i == 0 else rates[i - 1]
            y = torch.nn.functional.conv2d(x, wt.double(), padding=0 if i == 0 else d, dilation=d)
            tot = tot + (y * G[..., i * cout:(i + 1) * cout].permute(0, 3, 1, 2).double()).sum()
        tot.backward()
        _OPERANDS[shape] = (G, ws, x.grad.permute(0, 2, 3, 1).contiguous())
    return _OPERANDS[shape]


def _device_operands(ops, shape):
    n, h, w, cin, cout, rates = SHAPES[shape]
    G, ws, _ = _operands(shape)
    Gd = G.to(DEV).view(n * h * w, -1)
    am_g = ops.amax_of(Gd)
    return Gd, am_g, ops.packed_of(Gd, am_g), [torch.nn.Parameter(t.to(DEV)) for t in ws]


def _one_launch(ops, shape, Gp, am_g, ws, dx, slot=None):
    """The segmented launch on packed operands made with ops.packed_of."""
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    segs = ops.aspp_dgrad_segments(rates, h, w, cout)
    Wd = ops.aspp_dgrad_weights(ws, segs)
    # the image itself: Wc's rows, then the tap slab of every segment
    want = [ws[0].detach()[:, :, 0, 0]] + [t.detach()[:, :, 1, 1] for t in ws[1:]] + [ws[i].detach()[:, :, t // 3, t % 3] for i, t, _, _, _ in segs]
    assert torch.equal(Wd, torch.cat(want, dim=0))
    WdT = Wd.t().contiguous()
    am_w = ops.amax_of(WdT)
    assert float(am_w) == float(Wd.abs().max()) == float(ops.amax_of(Wd))
    ok = ops.gemm("nt", Gp, ops.packed_of(WdT, am_w), dx, M=rows, N=cin, K=k * cout, lda=k * cout, ldb=Wd.shape[0], ldc=cin,
                  geo=(n, h, w, h, w, 1, 1, 1, 0, 1), amax_a=am_g, amax_b=am_w, amax_c=slot, a_packed=True, b_packed=True,
                  seg=(cout, [(oy, ox, acol) for _, _, oy, ox, acol in segs], 0.0, 0.0))
    assert ok, "the library refused the segmented launch"
    return len(segs)


def _three_launches(ops, shape, Gp, am_g, ws, dx):
    """The launches ops.AsppCentreFn.backward makes with the switch off, on the same packed gradient image."""
    from glfusion_amd import conv_plan
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    ldu = k * cout
    Wc = ops.aspp_centre_weights(ws)
    WcT, am_wc = Wc.t().contiguous(), ops.amax_of(Wc)
    ops.gemm("nt", Gp, ops.packed_of(WcT, am_wc), dx, M=rows, N=cin, K=ldu, lda=ldu, ldb=ldu, ldc=cin, amax_a=am_g, amax_b=am_wc,
             a_packed=True, b_packed=True)
    for i in range(1, k):
        d = rates[i - 1]
        pl = conv_plan.plan("dgrad", (n, h, w, cin, cout, 3, 3, 1, d, d), ops.PRECISIONS.index(ops.get_precision()), keep=~ops.CENTRE_TAP)
        off, rect = pl.mask, pl.rect
        if not off:
            continue
        assert rect in (0, 2)                  # (dense or regions: both accumulate into dx without atomics)
        wT = ws[i].detach().permute(2, 3, 1, 0).reshape(9, cin, cout).contiguous()
        am_w = ops.amax_of(wT)
        ops.gemm("nt", Gp[:, i * cout:(i + 1) * cout], ops.packed_of(wT, am_w), dx, M=rows, N=cin, K=cout, lda=ldu, ldb=cout, ldc=cin,
                 taps=9, mask=off, tap_stride_b=cout * cin, gather=2, geo=(n, h, w, h, w, 3, 3, 1, d, d), rect=rect, accumulate=True,
                 amax_a=am_g, amax_b=am_w, a_packed=True, b_packed=True)


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_segmented_launch_against_float64(shape, prec):
    """Kernel level, plus the single-store, reproducibility and amax properties of the same launch."""
    from glfusion_amd import ops
    n, h, w, cin, cout, rates = SHAPES[shape]
    want = _operands(shape)[2].view(-1, cin)
    rows = n * h * w
    with ops.precision_scope(prec):
        Gd, am_g, Gp, ws = _device_operands(ops, shape)
        # single store: no NaN survives, and nothing is read from dx -- two finite prefills give the same bits
        slot = ops.amax_slot(DEV)
        a = torch.full((rows, cin), float("nan"), device=DEV)
        nseg = _one_launch(ops, shape, Gp, am_g, ws, a, slot)
        b = torch.full((rows, cin), 3.0e30, device=DEV)
        _one_launch(ops, shape, Gp, am_g, ws, b)
        c = torch.full((rows, cin), -7.25, device=DEV)
        _one_launch(ops, shape, Gp, am_g, ws, c)
        old = torch.empty(rows, cin, device=DEV)
        _three_launches(ops, shape, Gp, am_g, ws, old)
        torch.cuda.synchronize()
        ops.reset_weight_images()
    assert nseg > 0
    assert not bool(torch.isnan(a).any()), "an output element was not stored"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    # the reported maximum is the maximum of what was stored
    true = float(a.abs().max())
    assert abs(float(slot) - true) <= 1e-6 * true, (float(slot), true)
    e_one, e_old = _rel(a, want), _rel(old, want)
    print(f"{shape} {prec} nseg {nseg}: one launch {e_one:.3e} three launches {e_old:.3e} ratio {e_one / max(e_old, 1e-30):.3f}")
    assert e_one <= 1.5 * e_old + 1e-7, (e_one, e_old)


def _step(shape, prec, one):
    """One train step of models.deeplabv3.ASPP (the centre-tap route on) with the switch set; the tensors
    test_gpu_aspp_centre.py compares, and the keyword arguments of every contraction AsppCentreFn.backward issued."""
    from glfusion_amd import ops
    keep = (ops.ASPP_DGRAD_ONE, ops.AsppCentreFn.backward, ops.gemm)
    calls, inside = [], [False]

    def gemm_spy(mode, *a, **kw):
        if inside[0]:
            calls.append((mode, dict(kw)))
        return keep[2](mode, *a, **kw)

    def bwd_spy(ctx, *dys):
        inside[0] = True
        try:
            return keep[1](ctx, *dys)
        finally:
            inside[0] = False
    try:
        ops.ASPP_DGRAD_ONE, ops.AsppCentreFn.backward, ops.gemm = one, staticmethod(bwd_spy), gemm_spy
        out, launches, _ = base._run(MODULE_SHAPES[shape], prec, True)
        with ops.precision_scope(prec):
            ops.reset_weight_images()
        return out, launches, calls
    finally:
        ops.ASPP_DGRAD_ONE, ops.gemm = keep[0], keep[2]
        ops.AsppCentreFn.backward = staticmethod(keep[1])


def _dgrad_calls(calls, cin, rows):
    return [kw for mode, kw in calls if mode == "nt" and kw["N"] == cin and kw["M"] == rows]


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_train_step_switch_on_against_off(shape, prec):
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    want = base._oracle(MODULE_SHAPES[shape])[3]
    on, launches_on, calls_on = _step(shape, prec, True)
    off, launches_off, calls_off = _step(shape, prec, False)
    # on: exactly one NT launch with N = Cin in AsppCentreFn.backward, a segmented one, and nothing accumulates
    d_on = _dgrad_calls(calls_on, cin, rows)
    assert len(d_on) == 1 and d_on[0].get("seg") is not None and d_on[0]["K"] == k * cout and d_on[0].get("taps", 1) == 1
    assert not any(kw.get("accumulate") for _, kw in calls_on)
    prof_on = [s for nm, s in launches_on if "gemm_rows_kernel<0" in nm and s[0] == rows and s[1] == cin]
    assert prof_on == [(rows, cin, k * cout, 1, 1, 1, 1, 0, 1)], prof_on
    # off: the stacked launch, then one launch per branch that keeps off-centre taps
    kept = [d for d in rates if ops_mask(h, w, d)]
    d_off = _dgrad_calls(calls_off, cin, rows)
    assert [kw.get("taps", 1) for kw in d_off] == [1] + [9] * len(kept) and all(kw.get("seg") is None for kw in d_off)
    assert [kw["geo"][9] for kw in d_off[1:]] == kept and [kw["mask"] for kw in d_off[1:]] == [ops_mask(h, w, d) for d in kept]
    assert len([s for nm, s in launches_off if "gemm_rows_kernel<0" in nm and s[0] == rows and s[1] == cin]) == 1 + len(kept)
    worst = 0.0
    for key, ref in want.items():
        if key.endswith("num_batches_tracked"):
            assert int(on[key]) == int(ref) == int(off[key]), key
            continue
        e_on, e_off = base._rel(on[key], ref), base._rel(off[key], ref)
        print(f"{shape} {prec} {key}: one launch {e_on:.3e} off {e_off:.3e}")
        worst = max(worst, e_on / max(e_off, 1e-30))
        assert e_on <= 1.5 * e_off + 1e-7, (key, e_on, e_off)
    print(f"{shape} {prec}: largest on / off error ratio {worst:.3f}")


def ops_mask(h, w, d):
    from glfusion_amd import ops
    return ops.tap_mask(2, h, w, h, w, 3, 3, 1, d, d) & ~ops.CENTRE_TAP


def test_environment_switch():
    """GLF_ASPP_DGRAD_ONE=0 turns the route off at import, like its two siblings; unset, it is on."""
    code = "from glfusion_amd import ops; print(int(ops.ASPP_DGRAD_ONE), int(ops.ASPP_CENTRE), int(ops.ASPP_CENTRE_WGRAD))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "GLF_ASPP_DGRAD_ONE"}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    for value, want in ((None, "1 1 1"), ("0", "0 1 1"), ("1", "1 1 1")):
        e = dict(env) if value is None else dict(env, GLF_ASPP_DGRAD_ONE=value)
        e.pop("GLF_ASPP_CENTRE", None)
        e.pop("GLF_ASPP_CENTRE_WGRAD", None)
        got = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split("\n")[-2]
        assert got == want, (value, got)
