"""GPU: glf_cps_bce_sum (csrc/pointwise.hip), the cross pseudo supervision loss, through its C entry point and through the autograd
node ops.cps_bce_sum, against the float64 restatement tests/cps_ref.cps_ref on the same inputs.

Inputs: pointwise_ref.bce_inputs logits (two seeds) with the sign pairs (0, 0), (0, +), (+, 0), (-, +) planted in front; both
satisfy pointwise_ref.overlap_condition, so `x > 0` and the device predicate sigmoid(x) > 0.5 agree on every element.  Sizes:
pointwise_ref.BCE_NUMEL, one size whose scalar grid-stride loop takes a second, ragged trip (pointwise_ref.big) and four times
that plus 3 (the same for the 16-byte loop, with a tail); each once with every base on a 16-byte boundary and once with both
inputs and both gradients one element past it (the scalar path).

Gates: stats bit for bit; the loss by pointwise_ref's gate at K_BCE on the reference's magnitude (the per-element arithmetic is
bce_kernel's, the two directions meet in double); da / db at K_BCE_DX with the TINY |g| floor and again without it where
|x| <= 80, as the BCE test.  Every output sits in a guarded buffer."""
import pytest
import torch

import cps_ref as CR
import pointwise_ref as R
from pointwise_ref import DEV, F32, F64, GUARD, Guarded, gate, ptr

pytestmark = pytest.mark.gpu

ERR_BAD_SHAPE, ERR_NULL = -1, -5      # include/glfusion.h


class Shifted(Guarded):
    """A guarded [1][c] buffer whose live part starts `off` elements past a 16-byte boundary."""

    def __init__(self, c, off, dtype=F32):
        self.sent, self.off = self.SENT[dtype], off
        self.buf = torch.full((GUARD + off + c + GUARD,), self.sent, dtype=dtype, device=DEV)
        self.body = self.buf[GUARD + off:GUARD + off + c].view(1, c)
        self.t = self.body
        self.rows, self.ld, self.c = 1, c, c
        assert self.ptr % 16 == (off * self.buf.element_size()) % 16

    def intact(self):
        lo, hi = GUARD + self.off, GUARD + self.off + self.c
        return bool((self.buf[:lo] == self.sent).all()) and bool((self.buf[hi:] == self.sent).all())


def shifted_input(values, off):
    """fp32 copy of float64 `values` on the device, `off` elements past a 16-byte boundary; NaN around it"""
    n = values.numel()
    base = torch.full((4 + off + n + 4,), float("nan"), dtype=F32, device=DEV)
    t = base[4 + off:4 + off + n]
    t.copy_(values)
    assert torch.equal(t.double().cpu(), values), "input is not an fp32 value"
    assert t.data_ptr() % 16 == 4 * off
    return t


@pytest.fixture(scope="module")
def L():
    from glfusion_amd._lib import lib, check
    return lib, check


@pytest.fixture(scope="module")
def SIZES():
    big = R.big(torch.cuda.get_device_properties(0).multi_processor_count)
    return R.BCE_NUMEL + [big, 4 * big + 3]


_CASES = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    """the shared references live on the device: give the memory back when the module is done"""
    yield
    _CASES.clear()
    torch.cuda.empty_cache()


def case(numel):
    """inputs and float64 references of one size, computed once and shared (never modified)"""
    if numel not in _CASES:
        a, b = CR.plant_pairs(R.bce_inputs(numel, seed=601)[0], R.bce_inputs(numel, seed=641)[0])
        assert R.overlap_condition(a) and R.overlap_condition(b)
        ad, bd = a.to(DEV), b.to(DEV)
        refs = {g: CR.cps_ref(ad, bd, g) for g in (1.0 / 64, 0.25 / 64)}
        _CASES[numel] = (a, b, ad, bd, refs)
    return _CASES[numel]


def guards(*bufs, what=""):
    for g in bufs:
        assert g.intact(), f"{what}: a guard element was overwritten"
        assert g.written(), f"{what}: an element was not written"


def gate_grads(da, db, ad, bd, ref, g, what):
    _, _, dar, dam, dbr, dbm, _ = ref
    for got, want, mag, x, name in ((da, dar, dam, ad, "da"), (db, dbr, dbm, bd, "db")):
        got, want, mag, x = got.reshape(1, -1).double(), want.reshape(1, -1), mag.reshape(1, -1), x.reshape(1, -1)
        gate(got, want, mag, R.K_BCE_DX, False, f"{what} {name}", "cps " + name, extra=torch.full_like(mag, R.TINY * abs(g)))
        gate(got, want, mag, R.K_BCE_DX, False, f"{what} {name}", f"cps {name}, |x| <= 80", sure=x.abs() <= 80)


@pytest.mark.parametrize("off", [0, 1])
def test_cps_bce_sum_kernel(L, SIZES, off):
    lib, check = L
    for numel in SIZES:
        a, b, ad, bd, refs = case(numel)
        ab, bb = shifted_input(a, off), shifted_input(b, off)
        for gdev in (None, 0.25):
            gs = 1.0 / 64
            g = gs * (gdev or 1.0)
            lref, lmag, _, _, _, _, sref = refs[g]
            gsd = None if gdev is None else torch.tensor([gdev], dtype=F32, device=DEV)
            da, db = Shifted(numel, off), Shifted(numel, off)
            for bwd in (False, True):
                what = f"cps {numel} off {off} bwd {bwd} grad_scale_dev {gdev}"
                loss, stats = Guarded(1, 1, dtype=F64), Guarded(1, 4, dtype=torch.int64)
                check(lib.glf_cps_bce_sum(ptr(ab), ptr(bb), loss.ptr, stats.ptr, ptr(da) if bwd else None, ptr(db) if bwd else None,
                                          gs, ptr(gsd), numel, None), "cps_bce_sum")
                torch.cuda.synchronize()
                guards(loss, stats, what=what)
                assert torch.equal(stats.t[0].cpu(), sref), f"{what}: stats {stats.t[0].tolist()} != {sref.tolist()}"
                print(f"{what}: loss {float(loss.t[0, 0])!r} ref {float(lref)!r} |diff| / d {abs(float(loss.t[0, 0]) - float(lref)) / float(R.tol(R.K_BCE, lmag)):.3g}")
                gate(loss.f64(), lref.view(1, 1), lmag.view(1, 1), R.K_BCE, False, what + " loss", "cps loss")
                if not bwd:
                    assert da.untouched() and db.untouched(), what + ": a forward call wrote a gradient"
                else:
                    guards(da, db, what=what)
                    gate_grads(da.t, db.t, ad, bd, refs[g], g, what)
            # stats may be NULL
            loss = Guarded(1, 1, dtype=F64)
            check(lib.glf_cps_bce_sum(ptr(ab), ptr(bb), loss.ptr, None, None, None, gs, None, numel, None), "cps_bce_sum")
            torch.cuda.synchronize()
            guards(loss, what="no stats")
            gate(loss.f64(), lref.view(1, 1), lmag.view(1, 1), R.K_BCE, False, f"cps {numel} off {off} no stats: loss", "cps loss")


def test_cps_stats_are_overlap_counts_of_the_hard_labels(L):
    """bit for bit what glf_overlap_counts(a, on(b)) returns (on(b) = b > 0 under overlap_condition)"""
    lib, check = L
    numel = 4099
    _, _, ad, bd, _ = case(numel)
    af, bf = ad.float(), bd.float()
    onb = (bf > 0).float()
    loss, stats, counts = Guarded(1, 1, dtype=F64), Guarded(1, 4, dtype=torch.int64), Guarded(1, 4, dtype=torch.int64)
    check(lib.glf_cps_bce_sum(ptr(af), ptr(bf), loss.ptr, stats.ptr, None, None, 1.0, None, numel, None), "cps_bce_sum")
    check(lib.glf_overlap_counts(ptr(af), ptr(onb), counts.ptr, numel, None), "overlap_counts")
    torch.cuda.synchronize()
    assert torch.equal(stats.t, counts.t) and int(stats.t.sum()) == numel


def test_cps_bce_sum_refusals_on_device_pointers(L):
    lib, _ = L
    z, y = torch.zeros(8, dtype=F32, device=DEV), torch.zeros(8, dtype=F32, device=DEV)
    loss, stats, da, db = Guarded(1, 1, dtype=F64), Guarded(1, 4, dtype=torch.int64), Guarded(1, 8), Guarded(1, 8)
    bufs = (loss, stats, da, db)

    def refused(rc, status, fragment):
        msg = lib.glf_last_error().decode()
        assert rc == status and fragment in msg, (rc, status, fragment, msg)
        torch.cuda.synchronize()
        assert all(g.untouched() for g in bufs), "a refused call wrote: " + fragment
        assert not bool(z.any()) and not bool(y.any())

    call = lambda a, b, l, st, ga, gb, n: lib.glf_cps_bce_sum(a, b, l, st, ga, gb, 1.0, None, n, None)
    refused(call(None, ptr(y), loss.ptr, stats.ptr, None, None, 8), ERR_NULL, "cps_bce_sum: null argument")
    refused(call(ptr(z), None, loss.ptr, stats.ptr, None, None, 8), ERR_NULL, "cps_bce_sum: null argument")
    refused(call(ptr(z), ptr(y), None, stats.ptr, None, None, 8), ERR_NULL, "cps_bce_sum: null argument")
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, da.ptr, None, 8), ERR_NULL, "cps_bce_sum: null argument")
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, None, db.ptr, 8), ERR_NULL, "cps_bce_sum: null argument")
    refused(call(ptr(z), None, loss.ptr, stats.ptr, da.ptr, da.ptr, 0), ERR_NULL, "cps_bce_sum: null argument")       # null wins
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, None, None, 0), ERR_BAD_SHAPE, "cps_bce_sum: numel must be > 0")
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, da.ptr, db.ptr, -4), ERR_BAD_SHAPE, "cps_bce_sum: numel must be > 0")
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, ptr(z), db.ptr, 8), ERR_BAD_SHAPE, "cps_bce_sum: outputs must not alias")
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, da.ptr, ptr(y), 8), ERR_BAD_SHAPE, "cps_bce_sum: outputs must not alias")
    refused(call(ptr(z), ptr(y), loss.ptr, stats.ptr, da.ptr, da.ptr, 8), ERR_BAD_SHAPE, "cps_bce_sum: outputs must not alias")


def test_cps_autograd_node():
    """(0.37 * ops.cps_bce_sum(a, b)).backward() on [2,5,9,11] logits: both gradients within the kernel's gates, the upstream scalar
    read on the device; with b detached only a gets one; stats are filled by the forward."""
    from glfusion_amd import ops
    shape = (2, 5, 9, 11)
    numel = 2 * 5 * 9 * 11
    a64, b64, ad, bd, _ = case(numel)
    g = float(torch.tensor(0.37, dtype=F32))                # the upstream gradient is an fp32 scalar
    ref = CR.cps_ref(ad, bd, g)
    a = ad.float().view(shape).requires_grad_(True)
    b = bd.float().view(shape).requires_grad_(True)
    stats = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    loss = ops.cps_bce_sum(a, b, stats)
    assert loss.dtype == F32 and loss.dim() == 0
    (0.37 * loss).backward()
    torch.cuda.synchronize()
    assert torch.equal(stats.cpu(), ref[6])
    # the fp32 scalar: the double sum (gated by the kernel test) rounded once
    lref, lmag = CR.cps_ref(ad, bd, 1.0)[:2]
    assert abs(float(loss.detach()) - float(lref)) <= float(R.tol(R.K_BCE + 1, lmag))
    gate_grads(a.grad, b.grad, ad, bd, ref, g, "autograd node")

    a2 = ad.float().view(shape).requires_grad_(True)
    b2 = bd.float().view(shape).requires_grad_(True)
    (0.37 * ops.cps_bce_sum(a2, b2.detach())).backward()
    torch.cuda.synchronize()
    assert b2.grad is None
    assert torch.equal(a2.grad, a.grad)                     # the labels are constants: a's gradient never came through b
    with pytest.raises(RuntimeError, match="shape"):
        ops.cps_bce_sum(a2, b2[:, :4])
