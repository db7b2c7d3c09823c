"""The ASPP centre taps' WEIGHT gradients as one stacked contraction (ops.AsppCentreFn.backward with ops.ASPP_CENTRE_WGRAD):
the stacked route against the per-branch route (flag off), both judged by the oracle's ASPP in float64 on the CPU.

Yardstick (that of test_gpu_aspp_centre.py, for the same reason): for every conv-weight gradient the stacked route's relative L2
error against float64 must be <= 1.5 x the per-branch route's error against the same float64 result, + 1e-7.  The two routes add
the same products in another slice order -- the centre tap's full-map reduction is cut into the stacked launch's slices where
it was cut into the branch's own -- which 1.5 covers; a wrong row block, tap or scale misses it by orders of magnitude."""
import pytest
import torch

from oracle import glfusion_ref as orc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the shapes of test_gpu_aspp_centre.py: (a) rate 36 is centre-only, rate 12 / 24 keep eight off-centre taps as rectangles;
# (b) a non-square map, rate 12 >= both extents (centre-only); (c) no branch whose forward sums with float atomics: two runs agree
# bit for bit
SHAPES = {"a": (3, 28, 28, 64, 32, (12, 24, 36)), "b": (2, 12, 10, 64, 32, (3, 6, 12)), "c": (2, 12, 10, 64, 32, (1, 1, 12))}
CENTRE = 1 << 4
WKEYS = [f"convs.{i}.0.weight" for i in range(4)]


def _rel(a, ref):
    ref = ref.double()
    return float((a.detach().cpu().double() - ref).norm()) / max(float(ref.norm()), 1e-300)


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


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
    """float64 conv-weight gradients, computed once per shape and shared."""
    if shape not in _ORACLE:
        ref, x, up = _state(shape)
        sd = {k: v.clone() for k, v in ref.state_dict().items()}
        ref = ref.double().train()
        y = ref(x.double())
        (y * up.double()).sum().backward()
        _ORACLE[shape] = (sd, x, up, {k: dict(ref.named_parameters())[k].grad for k in WKEYS})
    return _ORACLE[shape]


def _run(shape, prec, stacked, slots=None):
    """One train step of the HIP ASPP from the shared state: the conv-weight gradients, the TN launches ops.PROFILER saw as
    (M, N, K, taps, kept taps, dilation), and (dilation, tap mask) of every 9-tap TN call -- an empty mask is the store-only
    form, which contracts nothing."""
    from glfusion_amd import ops
    from glfusion_amd.models.deeplabv3 import ASPP
    n, h, w, cin, cout, rates = SHAPES[shape]
    sd, x, up, _ = _oracle(shape)
    keep, masks = (ops.ASPP_CENTRE_WGRAD, ops.PROFILER, ops.gemm), []
    try:
        ops.ASPP_CENTRE_WGRAD = stacked
        assert ops.ASPP_CENTRE
        with ops.precision_scope(prec):
            m = ASPP(cin, list(rates), cout)
            m.load_state_dict(sd, strict=True)
            orc.set_dropout(m, 0.0)
            m = m.to(DEV).train()
            if slots is not None:
                slots(m)

            def spy(mode, *a, **k):
                if mode == "tn" and k.get("taps", 1) == 9:
                    masks.append((k["geo"][9], k["mask"]))
                return keep[2](mode, *a, **k)
            ops.gemm = spy
            ops.PROFILER = prof = []
            xg = x.to(DEV).requires_grad_(True)
            assert ops.aspp_centre_ok(ops.to_nhwc(xg), [cv[0] for cv in m.convs[:-1]])
            y = m(xg)
            (y * up.to(DEV)).sum().backward()
            torch.cuda.synchronize()
        grads = {k: dict(m.named_parameters())[k].grad for k in WKEYS}
        tn = [(s[0], s[1], s[2], s[3], s[4], s[8]) for nm, s in ((p[0], p[5]) for p in prof) if nm.startswith("gemm_tn")]
        return grads, tn, masks, m
    finally:
        ops.ASPP_CENTRE_WGRAD, ops.PROFILER, ops.gemm = keep


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_stacked_route_against_per_branch_route(shape, prec):
    from glfusion_amd import ops
    n, h, w, cin, cout, rates = SHAPES[shape]
    want = _oracle(shape)[3]
    k, rows = 1 + len(rates), n * h * w
    on, tn_on, masks_on, _ = _run(shape, prec, True)
    off, tn_off, masks_off, _ = _run(shape, prec, False)
    # accuracy
    for key in WKEYS:
        e_on, e_off = _rel(on[key], want[key]), _rel(off[key], want[key])
        print(f"{shape} {prec} {key}: stacked {e_on:.3e} per-branch {e_off:.3e}")
        assert e_on <= 1.5 * e_off + 1e-7, (key, e_on, e_off)
    # launch census
    full = {d: ops.tap_mask(1, h, w, h, w, 3, 3, 1, d, d) for d in rates}
    n_off_centre = sum(1 for d in rates if full[d] & ~CENTRE)
    assert n_off_centre < len(rates)                             # every shape has a centre-only branch
    stacked = [s for s in tn_on if s[:4] == (k * cout, cin, rows, 1)]
    assert len(stacked) == 1, tn_on
    assert not [s for s in tn_on if s[:4] == (cout, cin, rows, 1)]                 # the 1x1 branch launches nothing of its own
    nine_on = [s for s in tn_on if s[3] == 9]
    assert len(nine_on) == n_off_centre, (tn_on, masks_on)                         # none for a centre-only branch ...
    assert sorted(d for d, mask in masks_on if not mask) == sorted(d for d in rates if not full[d] & ~CENTRE)      # ... only the store
    for d, mask in masks_on:
        assert not mask & CENTRE and mask == full[d] & ~CENTRE
    for s in nine_on:
        assert s[:3] == (cout, cin, rows) and s[4] == bin(full[s[5]]).count("1") - 1
    # flag off: none of this
    assert not [s for s in tn_off if s[:4] == (k * cout, cin, rows, 1)]
    assert len([s for s in tn_off if s[:4] == (cout, cin, rows, 1)]) == 1
    assert len([s for s in tn_off if s[3] == 9]) == len(rates) == len(masks_off)
    assert all(mask & CENTRE and mask == full[d] for d, mask in masks_off)


def _bucket(flat, held, shift=0):
    """One flat buffer registered as the gradient slots of the four branches' conv weights -- what ddp.GradAllReducer registers
    on a multi-rank job.  shift: floats before the first slot (1: no slot is 16-byte aligned)."""
    from glfusion_amd import ops

    def slots(m):
        named = [(key, dict(m.named_parameters())[key]) for key in WKEYS]
        buf = torch.zeros(shift + sum(p.numel() for _, p in named), device=DEV)
        o = shift
        for name, p in named:
            ops.register_grad_slot(p, buf, o)
            flat[name] = (o, p.numel())
            o += p.numel()
        held.extend(p for _, p in named)
        flat["buf"] = buf
    return slots


def test_two_runs_agree_bit_for_bit():
    a, _, _, _ = _run("c", "f16x3", True)
    b, _, _, _ = _run("c", "f16x3", True)
    for key in WKEYS:
        assert _bits(a[key], b[key]), key


@pytest.mark.parametrize("shift", [0, 1])                      # 1: the slots are not 16-byte aligned -- the tap-major route assembles them
def test_bucket_slots_get_the_same_gradients(shift):
    from glfusion_amd import ops
    flat, held = {}, []
    try:
        plain, _, _, _ = _run("c", "f16x3", True)
        inb, tn, _, m = _run("c", "f16x3", True, _bucket(flat, held, shift))
        assert len([s for s in tn if s[3] == 1 and s[0] == 4 * 32]) == 1
        for key in WKEYS:
            o, nel = flat[key]
            assert inb[key].data_ptr() == flat["buf"].data_ptr() + 4 * o, key      # the gradient IS the slot
            assert _bits(flat["buf"][o:o + nel], plain[key].reshape(-1)), key
    finally:
        ops.unregister_grad_slots(held)
