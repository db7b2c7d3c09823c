"""The forward of an ASPP head's four conv branches as ONE segmented launch with column groups (glf_gemm_nt_seg_cols,
ops.ASPP_FWD_ONE) against the launches it replaces: the stacked centre contraction plus one adding launch per branch that keeps
off-centre taps (per-tap rectangles with float atomics, or a dense accumulating launch).

Yardstick (the one test_gpu_aspp_centre.py and test_gpu_aspp_dgrad_one.py use): against a float64 result on the CPU computed
from the same operand values, the one launch's relative L2 error must be <= 1.5 x the replaced launches' error + 1e-7.  Both
routes sum the same products; the one launch does it under ONE weight scale (the maximum of the stacked image, at most the
largest branch maximum: one or two split bits lost for the other branches) and in one chain instead of rounded partial results.
A wrong offset, column group or region misses the bound by orders of magnitude.  Both errors are printed.

Cin = 64: two K-steps per segment, so the in-segment step and the segment change both run.  Cout = 128: the smallest column
group, one column tile per branch."""
import os
import subprocess
import sys

import pytest
import torch

import test_gpu_aspp_centre as base                              # the shared float64 oracle, the train-step runner and its yardstick

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (n, h, w, Cin, Cout, rates).  d: 24 segments, 5 x 7 bands on a non-square map.  a: the model's band structure (ragged tiles, rate
# 24's interior empty, rate 36 centre-only).  b: one rate >= both extents of a non-square map.
SHAPES = {"d": (2, 9, 12, 64, 128, (2, 4, 7)), "a": (3, 28, 28, 64, 128, (12, 24, 36)), "b": (2, 12, 10, 64, 128, (3, 6, 12))}
MODULE_SHAPES = {s: "fwd_one_" + s for s in SHAPES}              # keys of the shared oracle
for _s, _k in MODULE_SHAPES.items():
    base.SHAPES.setdefault(_k, SHAPES[_s])
GUARD = 64                                                       # sentinel rows in front of and behind U


def _rel(a, ref):
    return float((a.detach().cpu().double() - ref).norm()) / max(float(ref.norm()), 1e-300)


_OPERANDS = {}


def _operands(shape):
    """x [n, h, w, Cin], the four weights and the float64 outputs [rows][k Cout] of the four convolutions, once per shape."""
    if shape not in _OPERANDS:
        n, h, w, cin, cout, rates = SHAPES[shape]
        g = torch.Generator().manual_seed(13)
        x = torch.randn(n, h, w, cin, generator=g)
        ws = [torch.randn(cout, cin, 1, 1, generator=g) * 0.7] + [torch.randn(cout, cin, 3, 3, generator=g) * (0.3 + 0.4 * i) for i in range(len(rates))]
        xd = x.permute(0, 3, 1, 2).double()
        us = []
        for i, wt in enumerate(ws):
            d = 1 if i == 0 else rates[i - 1]
            us.append(torch.nn.functional.conv2d(xd, wt.double(), padding=0 if i == 0 else d, dilation=d).permute(0, 2, 3, 1))
        _OPERANDS[shape] = (x, ws, torch.cat(us, dim=-1).reshape(n * h * w, -1).contiguous())
    return _OPERANDS[shape]


def _device_operands(ops, shape):
    x, ws, _ = _operands(shape)
    xd = x.to(DEV).view(-1, x.shape[-1])
    am_x = ops.amax_of(xd)
    return xd, am_x, ops.packed_of(xd, am_x), [torch.nn.Parameter(t.to(DEV)) for t in ws]


def _guarded(rows, ldu, fill):
    buf = torch.full((rows + 2 * GUARD, ldu), -1234.5, device=DEV)
    U = buf[GUARD:GUARD + rows]
    U.fill_(fill)
    return buf, U


def _one_launch(ops, shape, xp, am_x, ws, U, slot=None, sums=None, colmax=None):
    """The segmented launch on packed operands made with ops.packed_of."""
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    segs = ops.aspp_fwd_segments(rates, h, w, cout)
    Wf = ops.aspp_fwd_weights(ws, segs)
    # the image itself: Wc's rows, then the tap slab of every segment
    want = [ws[0].detach()[:, :, 0, 0]] + [t.detach()[:, :, 1, 1] for t in ws[1:]] + [ws[i].detach()[:, :, t // 3, t % 3] for i, t, _, _, _ in segs]
    assert torch.equal(Wf, torch.cat(want, dim=0))
    am_w = ops.amax_of(Wf)
    assert float(am_w) == float(Wf.abs().max())
    ok = ops.gemm("nt", xp, ops.packed_of(Wf, am_w), U, M=rows, N=k * cout, K=cin, lda=cin, ldb=cin, ldc=k * cout,
                  geo=(n, h, w, h, w, 1, 1, 1, 0, 1), amax_a=am_x, amax_b=am_w, amax_c=slot, colstats=sums, colmax=colmax,
                  a_packed=True, b_packed=True, seg=(cin, [(oy, ox, 0) for _, _, oy, ox, _ in segs], 0.0, 0.0),
                  seg_cols=ops.aspp_fwd_cols(segs, k, cout, cin))
    assert ok, "the library refused the segmented launch"
    return len(segs)


def _old_launches(ops, shape, xp, am_x, ws, U):
    """The launches ops.AsppCentreFn.forward makes with the switch off, on the same packed input image."""
    from glfusion_amd import conv_plan
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    ldu = k * cout
    Wc = ops.aspp_centre_weights(ws)
    am_wc = ops.amax_of(Wc)
    ops.gemm("nt", xp, ops.packed_of(Wc, am_wc), U, M=rows, N=ldu, K=cin, lda=cin, ldb=cin, ldc=ldu, amax_a=am_x, amax_b=am_wc,
             a_packed=True, b_packed=True)
    for i in range(1, k):
        d = rates[i - 1]
        pl = conv_plan.plan("fwd", (n, h, w, cin, cout, 3, 3, 1, d, d), ops.PRECISIONS.index(ops.get_precision()), keep=~ops.CENTRE_TAP)
        off, rect = pl.mask, pl.rect
        if not off:
            continue
        wt = ws[i].detach().permute(2, 3, 0, 1).reshape(9, cout, cin).contiguous()
        am_w = ops.amax_of(wt)
        ops.gemm("nt", xp, ops.packed_of(wt, am_w), U[:, i * cout:(i + 1) * cout], M=rows, N=cout, K=cin, lda=cin, ldb=cin, ldc=ldu,
                 taps=9, mask=off, tap_stride_b=cout * cin, gather=1, geo=(n, h, w, h, w, 3, 3, 1, d, d), rect=rect, accumulate=not rect,
                 amax_a=am_x, amax_b=am_w, a_packed=True, b_packed=True)


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_segmented_launch_against_float64(shape, prec):
    """Kernel level, plus the single-store, reproducibility, amax, colstats and colmax properties of the same launch."""
    from glfusion_amd import ops
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    ldu = k * cout
    want = _operands(shape)[2]
    with ops.precision_scope(prec):
        xd, am_x, xp, ws = _device_operands(ops, shape)
        # single store: no NaN survives, nothing outside U changes, nothing is read from U -- two prefills give the same bits
        slot_a, slot_b = ops.amax_slot(DEV), ops.amax_slot(DEV)
        sums, colmax = ops.stats_slot(ldu, DEV), ops.colmax_slot(ldu, DEV)
        buf_a, a = _guarded(rows, ldu, float("nan"))
        nseg = _one_launch(ops, shape, xp, am_x, ws, a, slot_a, sums, colmax)
        buf_b, b = _guarded(rows, ldu, 3.0e30)
        _one_launch(ops, shape, xp, am_x, ws, b, slot_b)
        old = torch.empty(rows, ldu, device=DEV)
        _old_launches(ops, shape, xp, am_x, ws, old)
        torch.cuda.synchronize()
        ops.reset_weight_images()
    assert nseg > 0
    assert not bool(torch.isnan(a).any()), "an output element was not stored"
    for buf in (buf_a, buf_b):
        assert bool((buf[:GUARD] == -1234.5).all()) and bool((buf[GUARD + rows:] == -1234.5).all()), "a store left U"
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(slot_a) == float(slot_b) == float(a.abs().max()), (float(slot_a), float(slot_b), float(a.abs().max()))
    # the fused statistics against float64 sums of the launch's own U (the tolerances of test_conv_epilogue_column_statistics)
    a2 = a.double()
    assert torch.allclose(sums[0], a2.sum(0), rtol=1e-6, atol=1e-6 * float(a2.abs().sum(0).max()))
    assert torch.allclose(sums[1], (a2 * a2).sum(0), rtol=1e-6)
    # a plain launch's colmax IS the column maxima of what it stored (test_bn_forward_writes_packed_activation): so is this one's
    assert torch.equal(colmax, a.abs().amax(dim=0))
    e_one, e_old = _rel(a, want), _rel(old, want)
    print(f"{shape} {prec} nseg {nseg}: one launch {e_one:.3e} replaced launches {e_old:.3e} ratio {e_one / max(e_old, 1e-30):.3f}")
    assert e_one <= 1.5 * e_old + 1e-7, (e_one, e_old)


def _step(shape_key, prec, one):
    """One train step of models.deeplabv3.ASPP (the centre-tap route on) with the switch set: the tensors test_gpu_aspp_centre.py
    compares, the contraction launches, the keyword arguments of every contraction AsppCentreFn.forward issued, the statistics
    ops.aspp_centre_convs handed out, and the number of statistics reduces (glf_bn_stats) of the step."""
    from glfusion_amd import ops, _lib
    dll = _lib.lib.load()
    keep = (ops.ASPP_FWD_ONE, ops.AsppCentreFn.forward, ops.gemm, ops.aspp_centre_convs, dll.glf_bn_stats)
    calls, inside, handed, reduces = [], [False], [], [0]

    def gemm_spy(mode, *a, **kw):
        if inside[0]:
            calls.append((mode, dict(kw)))
        return keep[2](mode, *a, **kw)

    def fwd_spy(ctx, *args):
        inside[0] = True
        try:
            return keep[1](ctx, *args)
        finally:
            inside[0] = False

    def convs_spy(*a, **kw):
        us, sums = keep[3](*a, **kw)
        handed.append([s is not None for s in sums])
        return us, sums

    def stats_spy(*a):
        reduces[0] += 1
        return keep[4](*a)
    try:
        ops.ASPP_FWD_ONE, ops.AsppCentreFn.forward, ops.gemm, ops.aspp_centre_convs = one, staticmethod(fwd_spy), gemm_spy, convs_spy
        dll.glf_bn_stats = stats_spy
        out, launches, _ = base._run(shape_key, prec, True)
        with ops.precision_scope(prec):
            ops.reset_weight_images()
        return out, launches, calls, handed, reduces[0]
    finally:
        ops.ASPP_FWD_ONE, ops.gemm, ops.aspp_centre_convs = keep[0], keep[2], keep[3]
        ops.AsppCentreFn.forward = staticmethod(keep[1])
        dll.glf_bn_stats = keep[4]


def _kept(h, w, rates):
    from glfusion_amd import ops
    return [d for d in rates if ops.tap_mask(1, h, w, h, w, 3, 3, 1, d, d) & ~ops.CENTRE_TAP]


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_train_step_switch_on_against_off(shape, prec):
    n, h, w, cin, cout, rates = SHAPES[shape]
    k, rows = 1 + len(rates), n * h * w
    want = base._oracle(MODULE_SHAPES[shape])[3]
    on, launches_on, calls_on, handed_on, reduces_on = _step(MODULE_SHAPES[shape], prec, True)
    off, launches_off, calls_off, handed_off, reduces_off = _step(MODULE_SHAPES[shape], prec, False)
    kept = _kept(h, w, rates)
    assert kept
    # on: the forward is exactly one contraction, a segmented one with column groups and fused statistics; every branch's
    # BatchNorm gets its sums, and the step makes one statistics reduce fewer per branch that keeps off-centre taps
    assert len(calls_on) == 1 and calls_on[0][0] == "nt"
    kw = calls_on[0][1]
    assert kw.get("seg") is not None and kw.get("seg_cols") is not None and kw["N"] == k * cout and kw["K"] == cin and kw["colstats"] is not None
    assert handed_on == [[True] * k]
    fwd_gather = lambda ls: [s for nm, s in ls if "gemm_rows_kernel<0,true>" in nm and s[0] == rows and s[1] == cout and s[2] == cin and s[3] == 9]
    stacked = lambda ls: [s for nm, s in ls if "gemm_rows_kernel<0,false>" in nm and s[0] == rows and s[1] == k * cout and s[2] == cin]
    assert len(stacked(launches_on)) == 1 and not fwd_gather(launches_on)
    # off: the stacked launch, then one launch per branch that keeps off-centre taps, whose BatchNorms reduce their own statistics
    assert [kw.get("taps", 1) for _, kw in calls_off] == [1] + [9] * len(kept) and all(kw.get("seg") is None for _, kw in calls_off)
    assert [kw["geo"][9] for _, kw in calls_off[1:]] == kept
    assert handed_off == [[True] + [d not in kept for d in rates]]
    assert len(stacked(launches_off)) == 1 and len(fwd_gather(launches_off)) == len(kept)
    assert reduces_off - reduces_on == len(kept), (reduces_on, reduces_off)
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


def test_narrow_head_takes_the_other_route():
    """Cout = 32 is no whole column tile: with the switch on the head makes the stacked launch and the adding launches."""
    n, h, w, cin, cout, rates = base.SHAPES["b"]
    assert cout == 32
    _, launches, calls, handed, _ = _step("b", "f16x3", True)
    kept = _kept(h, w, rates)
    assert [kw.get("taps", 1) for _, kw in calls] == [1] + [9] * len(kept)
    assert all(kw.get("seg") is None and kw.get("seg_cols") is None for _, kw in calls)
    assert handed == [[True] + [d not in kept for d in rates]]


def test_environment_switch():
    """GLF_ASPP_FWD_ONE=0 turns the route off at import, like its siblings; unset, it is on."""
    code = "from glfusion_amd import ops; print(int(ops.ASPP_FWD_ONE), int(ops.ASPP_DGRAD_ONE), int(ops.ASPP_CENTRE))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("GLF_ASPP_FWD_ONE", "GLF_ASPP_DGRAD_ONE", "GLF_ASPP_CENTRE")}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    for value, want in ((None, "1 1 1"), ("0", "0 1 1"), ("1", "1 1 1")):
        e = dict(env) if value is None else dict(env, GLF_ASPP_FWD_ONE=value)
        got = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split("\n")[-2]
        assert got == want, (value, got)
