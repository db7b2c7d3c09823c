"""ASPP conv branches with their centre taps as one contraction (ops.AsppCentreFn, split-fp16 precisions): the fused route
against the switched-off route, both judged by the oracle's ASPP in float64 on the CPU with the same parameters and inputs.

Yardstick: for every tensor, the fused route's relative L2 error against float64 must be <= 1.5 x the switched-off route's
error against the same float64 result (+ 1e-7 for tensors whose error is zero).  The arithmetic is the same products summed in
another order, under a scale shared by the four branches (up to one lost split bit): 1.5 covers that, a wrong tap, slice or
scale misses it by orders of magnitude.  Both errors are printed."""
import pytest
import torch

from oracle import glfusion_ref as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (a) the model's band structure on 28x28: rate 24's interior region is empty once the centre tap is masked out, rate 36 is
#     centre-only; ragged last tiles everywhere.  (b) a non-square map, one rate >= both extents.
#     (c) for bit-for-bit comparisons between two runs: no branch whose forward sums its taps with float atomics.
SHAPES = {"a": (3, 28, 28, 64, 32, (12, 24, 36)), "b": (2, 12, 10, 64, 32, (3, 6, 12)), "c": (2, 12, 10, 64, 32, (1, 1, 12))}


def _rel(a, ref):
    ref = ref.double()
    return float((a.detach().cpu().double() - ref).norm()) / max(float(ref.norm()), 1e-300)


def _state(shape):
    n, h, w, cin, cout, rates = SHAPES[shape]
    ref = orc.ASPP(cin, rates, cout)
    orc.closed_form_fill(ref, salt=31)
    orc.set_dropout(ref, 0.0)
    g = torch.Generator().manual_seed(7)
    for m in ref.modules():
        if isinstance(m, torch.nn.BatchNorm2d):                  # non-trivial gamma / beta
            with torch.no_grad():
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(torch.rand(m.bias.shape, generator=g) - 0.5)
    x = torch.randn(n, cin, h, w, generator=g)
    up = torch.randn(n, cout, h, w, generator=g)
    return ref, x, up


_ORACLE = {}


def _oracle(shape):
    """float64 results, computed once per shape and shared."""
    if shape not in _ORACLE:
        ref, x, up = _state(shape)
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        ref = ref.double().train()
        xd = x.double().requires_grad_(True)
        xp = x.double().requires_grad_(True)                     # the pooled branch's copy: its gradient arrives separately
        us, outs = [], []
        for b in ref.convs[:-1]:
            u = b[0](xd)
            u.retain_grad()                                      # the gradient a branch's BatchNorm hands to its conv
            us.append(u)
            outs.append(b[2](b[1](u)))
        cat = torch.cat(outs + [ref.convs[-1](xp)], dim=1)
        y = ref.project(cat)
        (y * up.double()).sum().backward()
        out = {"cat": cat.detach(), "y": y.detach(), "dx": xd.grad + xp.grad}
        extra = {"dU": float(max(u.grad.abs().max() for u in us)), "dx_group": float(xd.grad.abs().max())}
        out.update({"grad:" + k: p.grad for k, p in ref.named_parameters()})
        out.update({"buf:" + k: v.clone() for k, v in ref.state_dict().items() if "running" in k or "tracked" in k})
        _ORACLE[shape] = (sd, x, up, out, extra)
    return _ORACLE[shape]


def _amax_slots_bound(ops, m, seen, extra, shape, prec):
    """The maxima the fused route reports for its own tensors bound them, and the two scales shared by four branches lose no
    more bits than a single layer's.
    Wc: the combined maximum of the four parameters is the exact maximum of the stacked image.
    G:  the packed image cannot be read back, so its scale is judged by the float64 maximum of the four BatchNorm input
        gradients.  The slot is the largest of four per-layer bounds, each of glf_bn_bwd's packed_dx = 1 form, which
        test_bn_backward_writes_packed_gradient holds to [1, 4] x the layer's maximum; so the same window holds for the largest
        (below by the error of the gradients that reach the layers: 1e-4 under f16x3; under f16 every operand of the two
        contractions upstream is rounded to 2^-11, 2^-9 covers them).
    dx: the slot the stacked dgrad and the accumulating launches raise holds the largest value any of them stored, so it bounds
        what the last of them left.  No upper limit follows from that; the ratio is printed."""
    ws = [conv[0].weight for conv in m.convs[:-1]]
    Wc = ops.aspp_centre_weights(ws)
    stack = torch.cat([ws[0].detach()[:, :, 0, 0]] + [t.detach()[:, :, 1, 1] for t in ws[1:]], dim=0)
    assert torch.equal(Wc, stack) and float(ops.amax_of(Wc)) == float(stack.abs().max())
    g = float(seen["G"])
    print(f"{shape} {prec} amax G: slot {g:.4e} float64 max {extra['dU']:.4e} ratio {g / extra['dU']:.3f}")
    slack = 1e-4 if prec == "f16x3" else 2.0 ** -9
    assert (1.0 - slack) * extra["dU"] <= g <= 4.0 * extra["dU"], (g, extra["dU"])
    slot, true = seen["dx"]
    print(f"{shape} {prec} amax dx: slot {slot} max {true:.4e} float64 max {extra['dx_group']:.4e}")
    if slot is not None:                                         # (None: a launch with atomics took part, dx is measured on use)
        assert slot >= true, (slot, true)


def _run(shape, prec, fused, slots=None):
    """One train step of the HIP ASPP from the shared state: every checked tensor, and the contraction launches it made."""
    from glfusion_amd import ops
    from glfusion_amd.models.deeplabv3 import ASPP
    n, h, w, cin, cout, rates = SHAPES[shape]
    sd, x, up, _, extra = _oracle(shape)
    keep, seen = (ops.ASPP_CENTRE, ops.PROFILER, ops.conv1x1_cat, ops.AsppCentreFn.backward, ops.FanOutFn.backward), {}
    try:
        ops.ASPP_CENTRE = fused
        with ops.precision_scope(prec):
            m = ASPP(cin, list(rates), cout)
            m.load_state_dict(sd, strict=True)
            orc.set_dropout(m, 0.0)
            m = m.to(DEV).train()
            if slots is not None:
                slots(m)

            def spy(weight, xs, *a, **k):
                seen["cat"] = torch.cat([t.detach().permute(0, 3, 1, 2) for t in xs], dim=1)
                seen["amax"] = [ops.amax_of(t) for t in xs]
                return keep[2](weight, xs, *a, **k)
            ops.conv1x1_cat = spy

            def group_bwd(ctx, *dys):                            # the shared scale of the packed image G
                res = keep[3](ctx, *dys)
                seen["G"] = ctx.group.amax
                return res

            def fan_bwd(ctx, *dys):                              # the group's input gradient before the pooled branch is added
                for d in dys:
                    if d is not None and getattr(d, "_glf_owned", False):
                        torch.cuda.synchronize()
                        hit = getattr(d, "_glf_amax", None)
                        seen["dx"] = (None if hit is None else float(hit[2]), float(d.abs().max()))
                return keep[4](ctx, *dys)
            ops.AsppCentreFn.backward, ops.FanOutFn.backward = staticmethod(group_bwd), staticmethod(fan_bwd)
            ops.PROFILER = prof = []
            xg = x.to(DEV).requires_grad_(True)
            y = m(xg)
            (y * up.to(DEV)).sum().backward()
            torch.cuda.synchronize()
            if fused:
                _amax_slots_bound(ops, m, seen, extra, shape, prec)
        out = {"cat": seen["cat"], "y": y.detach(), "dx": xg.grad}
        out.update({"grad:" + k: p.grad for k, p in m.named_parameters()})
        out.update({"buf:" + k: v.clone() for k, v in m.state_dict().items() if "running" in k or "tracked" in k})
        for am in seen["amax"]:                                  # the shared slot of the branch buffer bounds it
            assert am is not None and float(am) >= float(seen["cat"].abs().max())
        return out, [(p[0], p[5]) for p in prof], m
    finally:
        ops.ASPP_CENTRE, ops.PROFILER, ops.conv1x1_cat = keep[:3]
        ops.AsppCentreFn.backward, ops.FanOutFn.backward = staticmethod(keep[3]), staticmethod(keep[4])


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", ["a", "b"])
def test_fused_route_against_switched_off_route(shape, prec):
    n, h, w, cin, cout, rates = SHAPES[shape]
    want = _oracle(shape)[3]
    on, launches_on, _ = _run(shape, prec, True)
    off, launches_off, _ = _run(shape, prec, False)
    k = 1 + len(rates)
    stacked = lambda ls: [s for nm, s in ls if (s[1], s[2]) in ((k * cout, cin), (cin, k * cout)) and s[3] == 1]
    assert len(stacked(launches_on)) == 2, "the fused route was not taken: no stacked forward + dgrad launch"
    assert not stacked(launches_off)
    worst = 0.0
    for key, ref in want.items():
        if key.endswith("num_batches_tracked"):
            assert int(on[key]) == int(ref) == int(off[key]), key
            continue
        e_on, e_off = _rel(on[key], ref), _rel(off[key], ref)
        print(f"{shape} {prec} {key}: fused {e_on:.3e} off {e_off:.3e}")
        worst = max(worst, e_on / max(e_off, 1e-30))
        assert e_on <= 1.5 * e_off + 1e-7, (key, e_on, e_off)
    print(f"{shape} {prec}: largest fused / off error ratio {worst:.3f}")


@pytest.mark.parametrize("cout", [32, 64])                      # K x kept taps = 256 / 512: the 4-wave and the 8-wave kernel
def test_accumulating_region_launch_leaves_the_empty_region_alone(cout):
    """glf_gemm_nt with rect = 2, accumulate = 1 and the centre bit cleared on shape (a)'s rate-24 dgrad geometry: the 20x20 interior
    (centre tap only) gets no tiles -- bit-identical C -- and the border is C plus the masked-tap result, within 1 ulp."""
    from glfusion_amd import ops
    n, h, w, cin = SHAPES["a"][:4]
    d, rows = 24, n * h * w
    with ops.precision_scope("f16x3"):
        g = torch.Generator().manual_seed(3)
        dy = torch.randn(rows, cout, generator=g).to(DEV)
        wT = torch.randn(9, cin, cout, generator=g).to(DEV)
        c0 = torch.randn(rows, cin, generator=g).to(DEV)
        mask = ops.tap_mask(2, h, w, h, w, 3, 3, 1, d, d) & ~ops.CENTRE_TAP
        assert mask
        kw = dict(M=rows, N=cin, K=cout, lda=cout, ldb=cout, ldc=cin, taps=9, mask=mask, tap_stride_b=cout * cin, gather=2,
                  geo=(n, h, w, h, w, 3, 3, 1, d, d), rect=2, amax_a=ops.amax_of(dy), amax_b=ops.amax_of(wT))
        r = torch.zeros(rows, cin, device=DEV)
        ops.gemm("nt", dy, wT, r, **kw)
        c = c0.clone()
        ops.gemm("nt", dy, wT, c, accumulate=True, **kw)
        torch.cuda.synchronize()
    c, c0, r = (t.view(n, h, w, cin).cpu() for t in (c, c0, r))
    lo, hi = h - d, d                                            # rows / columns [4, 24): only the centre tap is in range
    assert torch.equal(c[:, lo:hi, lo:hi].view(torch.int32), c0[:, lo:hi, lo:hi].view(torch.int32))
    assert float(r[:, lo:hi, lo:hi].abs().max()) == 0.0
    border = torch.ones(h, w, dtype=torch.bool)
    border[lo:hi, lo:hi] = False
    want = (c0 + r)[:, border]
    assert float(r[:, border].abs().min()) > 0.0
    assert bool(((c[:, border] - want).abs() <= want.abs() * 2.0 ** -23).all())


def test_weight_images_follow_the_parameters():
    """Wc / WcT are bit-identical to stacking slices of the parameters, follow an in-place update through ops.refresh_weights()
    and through a frozen table."""
    from glfusion_amd import ops
    g = torch.Generator().manual_seed(5)
    ws = [torch.nn.Parameter(torch.randn(32, 64, k, k, generator=g).to(DEV)) for k in (1, 3, 3, 3)]
    stack = lambda: torch.cat([ws[0].detach()[:, :, 0, 0]] + [t.detach()[:, :, 1, 1] for t in ws[1:]], dim=0)
    same = lambda a, b: torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    with ops.precision_scope("f16x3"):
        Wc = ops.aspp_centre_weights(ws)
        WcT = ops.weight_T(Wc, Wc)
        am = ops.amax_of(Wc)
        assert same(Wc, stack()) and same(WcT, stack().t()) and float(am) == float(stack().abs().max())
        with torch.no_grad():
            for t in ws:
                t.mul_(-1.5)
        ops.refresh_weights()
        assert ops.aspp_centre_weights(ws) is Wc and ops.weight_T(Wc, Wc) is WcT
        assert same(Wc, stack()) and same(WcT, stack().t()) and float(ops.amax_of(Wc)) == float(stack().abs().max())
        table = ops.freeze_weight_table(ws)
        with torch.no_grad():
            for t in ws:
                t.add_(0.25)
        ops.refresh_weights(frozen=table)
        torch.cuda.synchronize()
        assert same(Wc, stack()) and same(WcT, stack().t()) and float(am) == float(stack().abs().max())
        ops.reset_weight_images()


BIG = 3.0e30


def _bucket(flat, held, clobber=None):
    """Registers one flat buffer as the gradient slots of the four branches' conv weights and BatchNorm gamma / beta -- what
    ddp.GradAllReducer registers on a multi-rank job (with one rank it registers nothing).  clobber: a post-accumulate hook on
    every gamma / beta that keeps the finished gradient and then overwrites the slot, as a bucket's all-reduce may once the
    bucket's last gradient has arrived -- which is before the other branches' BatchNorm backward has run."""
    from glfusion_amd import ops

    def slots(m):
        named = [(f"convs.{i}.{j}.{nm}", getattr(conv[j], nm), j == 1) for i, conv in enumerate(m.convs[:-1])
                 for j, nm in ((0, "weight"), (1, "weight"), (1, "bias"))]
        buf = torch.zeros(sum(p.numel() for _, p, _ in named), device=DEV)
        o = 0
        for name, p, bn in named:
            ops.register_grad_slot(p, buf, o)
            flat[name] = (o, p.numel())
            o += p.numel()
            if clobber is not None and bn:
                def hook(q, name=name):
                    clobber[name] = q.grad.clone()
                    q.grad.fill_(BIG)
                    buf[flat[name][0]:flat[name][0] + flat[name][1]].fill_(BIG)
                p.register_post_accumulate_grad_hook(hook)
        held.extend(p for _, p, _ in named)
        flat["buf"] = buf
    return slots


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_bucket_slot_gets_the_same_gradients():
    """The branches' conv-weight, gamma and beta gradients written straight into registered all-reduce bucket slots equal, bit
    for bit, the same route writing to p.grad.  The slots are registered directly with ops.register_grad_slot and no
    ddp.GradAllReducer is attached: with one rank the reducer registers no slots, so attaching one would leave the
    in-bucket route untested."""
    from glfusion_amd import ops
    flat, held = {}, []
    try:
        plain, _, _ = _run("c", "f16x3", True)
        inb, _, m = _run("c", "f16x3", True, _bucket(flat, held))
        assert len(flat) == 13
        for name, v in flat.items():
            if name != "buf":
                assert _bits(flat["buf"][v[0]:v[0] + v[1]], plain["grad:" + name].reshape(-1)), name
        assert _bits(inb["dx"], plain["dx"])
    finally:
        ops.unregister_grad_slots(held)


def test_held_back_apply_passes_do_not_read_the_bucket():
    """A branch's gamma / beta gradients leave its BatchNorm backward node before the group's held-back apply passes run.  With
    their bucket slots overwritten at that moment the input gradient and every weight gradient are still, bit for bit, those of
    an undisturbed step, and the gamma / beta gradients taken before the overwrite are the undisturbed ones."""
    from glfusion_amd import ops
    flat, held, taken = {}, [], {}
    try:
        plain, _, _ = _run("c", "f16x3", True)
        hit, _, m = _run("c", "f16x3", True, _bucket(flat, held, taken))
        assert len(taken) == 8
        for name, g in taken.items():
            assert _bits(g, plain["grad:" + name]), name
            o, nel = flat[name]
            assert float(flat["buf"][o:o + nel].min()) == float(torch.tensor(BIG, dtype=torch.float32))
        for key, ref in plain.items():
            if key == "dx" or (key.startswith("grad:") and key[5:] not in taken):
                assert _bits(hit[key], ref), key
    finally:
        ops.unregister_grad_slots(held)


@pytest.mark.parametrize("shape", ["b", "c"])
def test_step_graph_replay_matches_eager_fused_step(shape):
    """One StepGraph capture and replay of the head: the replay's gradients equal the eager fused step's -- bit for bit on shape
    (c), where no forward launch sums with float atomics; on shape (b) rate 3 / 6 do, and two runs of the same step differ in
    the last bits of those branches."""
    from glfusion_amd import ops
    from glfusion_amd.engine import StepGraph
    from glfusion_amd.models.deeplabv3 import ASPP
    n, h, w, cin, cout, rates = SHAPES[shape]
    sd, x, up = _oracle(shape)[:3]
    ops.set_precision("f16x3")
    try:
        assert ops.ASPP_CENTRE
        xd, upd = x.to(DEV), up.to(DEV)

        def make():
            m = ASPP(cin, list(rates), cout)
            m.load_state_dict(sd, strict=True)
            orc.set_dropout(m, 0.0)
            m = m.to(DEV).train()
            params = list(m.parameters())

            def core():
                loss = (m(xd) * upd).sum()
                loss.backward()
                return loss.detach()
            return m, params, core
        m, params, core = make()
        assert ops.aspp_centre_ok(ops.to_nhwc(xd), [cv[0] for cv in m.convs[:-1]])
        want_loss = float(core())
        want = [p.grad.clone() for p in params]
        m2, params2, core2 = make()
        sg = StepGraph(core2, params2, warmup=2)
        for p in params2:
            p.grad = None
        loss = float(sg.replay())
        torch.cuda.synchronize()
        if shape == "c":
            assert loss == want_loss
            for (name, _), a, b in zip(m2.named_parameters(), params2, want):
                assert _bits(a.grad, b), name
        else:
            assert abs(loss - want_loss) <= 1e-6 * abs(want_loss)
            for a, b in zip(params2, want):
                assert float((a.grad - b).norm()) <= 1e-5 * float(b.norm()) + 1e-9
        sg.release()
    finally:
        ops.set_precision("f32")


def test_second_backward_through_the_same_graph():
    """retain_graph: a second backward pass through the fused head starts a round of its own in the gradient group (its own
    zeroed bound, its own count of layers), so it computes the same gradients again: every accumulated gradient is exactly
    twice the first pass's, on the atomics-free shape (c)."""
    from glfusion_amd import ops
    from glfusion_amd.models.deeplabv3 import ASPP
    n, h, w, cin, cout, rates = SHAPES["c"]
    sd, x, up = _oracle("c")[:3]
    with ops.precision_scope("f16x3"):
        m = ASPP(cin, list(rates), cout)
        m.load_state_dict(sd, strict=True)
        orc.set_dropout(m, 0.0)
        m = m.to(DEV).train()
        xg = x.to(DEV).requires_grad_(True)
        assert ops.ASPP_CENTRE and ops.aspp_centre_ok(ops.to_nhwc(xg), [cv[0] for cv in m.convs[:-1]])
        loss = (m(xg) * up.to(DEV)).sum()
        loss.backward(retain_graph=True)
        first = [xg.grad.clone()] + [p.grad.clone() for p in m.parameters()]
        loss.backward()
        torch.cuda.synchronize()
        for a, b in zip([xg.grad] + [p.grad for p in m.parameters()], first):
            assert _bits(a, b + b)
