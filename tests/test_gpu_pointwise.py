"""GPU: the pointwise kernels of csrc/pointwise.hip called through their C entry points, in both storages where both exist, and
judged element by element against float64 on the same inputs, every output in a guarded buffer: ReLU, axpby, add_n, the frame
copies / adds, dropout (against a host restatement of its counter hash), max-pool, the local gate, row sums and broadcasts, row
softmax, bilinear up-sampling, BCE / overlap counts, the 7x7 stem, the transposes and weight re-layouts, and their refusals.

Integer inputs are gated for equality, Gaussian ones by the interval d = (k + 4) 2^-23 magnitude with k counted from the kernel
source; selections and copies are always equality.  The derivations, shape lists and references are in tests/pointwise_ref.py,
their CPU side in tests/test_pointwise_ref_cpu.py.  One case per grid-stride kernel has CAP + 3 * 256 + 5 accesses (CAP = 8
workgroups of 256 threads per CU, from torch at run time), so every such loop makes a second, ragged trip.  The largest
|got - ref| / d per output is printed when the module finishes (recorded in profiles/pointwise_gate.txt)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import pointwise_ref as R
from pointwise_ref import BF, DEV, F32, F64, Guarded, Guarded16, GuardedMask, exact, gate, gate_rel, ptr, put, put32, put16, out_buf, vec32

pytestmark = pytest.mark.gpu

OK, ERR_BAD_SHAPE, ERR_UNSUPPORTED, ERR_NULL = 0, -1, -2, -5      # include/glfusion.h
DT_F32, DT_BF16 = 0, 1
STORAGES = ["f32", "bf16"]
FAMILIES = ["int", "gauss"]


@pytest.fixture(scope="module")
def L():
    from glfusion_amd._lib import lib, check
    yield lib, check
    for name, (n, worst, off) in sorted(R.RATIOS.items()):
        print(f"\nPOINTWISE_GATE {name}: tensors {n}, max |got - ref| / d {worst:.4g}, largest share != bf16_rne(ref) {off:.3g}", end="")
    print()


@pytest.fixture(scope="module")
def BIG():
    return R.big(torch.cuda.get_device_properties(0).multi_processor_count)


def sync():
    torch.cuda.synchronize()


def guards(*bufs, what=""):
    for g in bufs:
        if g is not None:
            assert g.intact(), f"{what}: a guard element or a pad column was overwritten"
            assert g.written(), f"{what}: an element was not written"


def fn(lib, st, name):
    return getattr(lib, ("glf_" if st == "f32" else "glf_s16_") + name)


def esize(st):
    return 4 if st == "f32" else 2


def refused(lib, rc, status, fragment, *bufs):
    msg = lib.glf_last_error().decode()
    assert rc == status and fragment in msg, (rc, status, fragment, msg)
    sync()
    assert all(g.untouched() for g in bufs), "a refused call wrote: " + fragment


def row(t):
    return t.reshape(1, -1)


def dev(t):
    return t.to(DEV)


def bf16_holds(ref):
    assert torch.equal(R.bf16_rne(ref), ref), "the integer case is not representable in bf16"


def judge(fam, st, got_buf, ref, mag, k, what, name):
    """equality in the integer family, the interval otherwise; got_buf: Guarded / Guarded16 whose .t has ref's element count"""
    ref, mag = dev(ref).reshape(got_buf.t.shape), dev(mag).reshape(got_buf.t.shape)
    if fam == "int":
        R.assert_exact(mag)
        if st == "bf16":
            bf16_holds(ref)
        exact(got_buf.dense(), ref, st == "bf16", what, name)
    else:
        gate(got_buf.f64(), ref, mag, k, st == "bf16", what, name)


# -------------------------------------------------------------------------------------------------------------------- relu
@pytest.mark.parametrize("st", STORAGES)
def test_relu_fwd_bwd(L, BIG, st):
    lib, check = L
    W = 1 if st == "f32" else 8
    for numel in R.RELU_NUMEL + [BIG * W]:
        x, dy = R.relu_inputs(st, numel)
        if numel % W:
            y = out_buf(st, 1, numel + 8)
            xb = put(st, row(torch.zeros(numel + 8, dtype=F64)))
            refused(lib, fn(lib, st, "relu_fwd")(ptr(xb), y.ptr, numel, None), ERR_BAD_SHAPE, "relu_fwd: numel must be a positive multiple of 8", y)
            refused(lib, fn(lib, st, "relu_bwd")(ptr(xb), ptr(xb), y.ptr, numel, None), ERR_BAD_SHAPE, "relu_bwd: numel must be a positive multiple of 8", y)
            continue
        xb, dyb = put(st, row(x)), put(st, row(dy))
        y, dx = out_buf(st, 1, numel), out_buf(st, 1, numel)
        check(fn(lib, st, "relu_fwd")(ptr(xb), y.ptr, numel, None), "relu_fwd")
        check(fn(lib, st, "relu_bwd")(ptr(dyb), ptr(xb), dx.ptr, numel, None), "relu_bwd")       # the mask is y > 0: x > 0 is the same set
        sync()
        what = f"{st} relu {numel}"
        guards(y, dx, what=what)
        exact(y.dense(), dev(row(R.relu_fwd_ref(x))), st == "bf16", what + " fwd", "relu y")
        exact(dx.dense(), dev(row(R.relu_bwd_ref(dy, x))), st == "bf16", what + " bwd", "relu dx")
        if numel <= 257:                                        # positive denormals and +inf pass through; nothing is flushed
            pos = x > 0
            assert torch.equal(y.f64()[0].cpu()[pos], x[pos]), what + ": a positive value (denormal, inf) did not pass unchanged"


# ------------------------------------------------------------------------------------------------------------------- axpby
def _axpby_case(L, st, fam, numel, a, b, off, what):
    lib, check = L
    if fam == "int":
        x, y = R.ints((numel,), 111, -3, 3), R.ints((numel,), 112, -3, 3)
    else:
        x, y = R.gaussian(st, (numel,), 113, 2.0, 0.3), R.gaussian(st, (numel,), 114, 1.0, -0.2)
    ox, oy, oo = off
    nanpad = lambda v, o: put(st, row(torch.cat([torch.zeros(o, dtype=F64), v])))
    xb, yb = nanpad(x, ox), nanpad(y, oy)
    live = torch.ones(numel + oo, dtype=torch.bool)
    live[:oo] = False
    out = GuardedMask(live, dtype=F32 if st == "f32" else torch.int16)
    es = esize(st)
    check(fn(lib, st, "axpby")(ptr(xb) + es * ox, ptr(yb) + es * oy, out.ptr + es * oo, a, b, numel, None), "axpby")
    sync()
    guards(out, what=what)
    ref, mag = R.axpby_ref(dev(x), dev(y), a, b)
    got = out.values()
    if fam == "int":
        R.assert_exact(mag)
        if st == "bf16":
            bf16_holds(ref)
        exact(got, ref, st == "bf16", what, "axpby out")
    else:
        gate(got.double(), ref, mag, R.K_AXPBY, st == "bf16", what, "axpby out")


@pytest.mark.parametrize("st", STORAGES)
def test_axpby(L, BIG, st):
    lib, _ = L
    ga, gb = float(np.float32(0.75)), float(np.float32(-1.3))
    offsets = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)] if st == "f32" else [(0, 0, 0)]
    for numel in R.AXPBY_NUMEL + ([1024, 1032] if st == "bf16" else []):
        if st == "bf16" and numel % 8:
            out = Guarded16(1, numel + 8)
            z = put16(row(torch.zeros(numel + 8, dtype=F64)))
            refused(lib, lib.glf_s16_axpby(ptr(z), ptr(z), out.ptr, 1.0, 1.0, numel, None), ERR_BAD_SHAPE, "s16_axpby: numel must be a positive multiple of 8", out)
            continue
        for off in offsets:
            for a, b in R.AXPBY_COEF:
                _axpby_case(L, st, "int", numel, a, b, off, f"{st} axpby int {numel} a {a} b {b} offsets {off}")
            _axpby_case(L, st, "gauss", numel, ga, gb, off, f"{st} axpby gauss {numel} offsets {off}")
    if st == "f32":
        # aligned: float4 body over a grid of at most 8192 workgroups (its own cap) + three single elements; x off by one: every
        # element singly, a grid of numel / 1024 workgroups walks it four times
        for numel, off in ((4 * (R.AXPBY_GRID + 3 * 256 + 5) + 3, (0, 0, 0)), (4 * BIG + 3, (1, 0, 0))):
            _axpby_case(L, st, "int", numel, 0.5, 2.0, off, f"f32 axpby int big {numel} offsets {off}")
            _axpby_case(L, st, "gauss", numel, ga, gb, off, f"f32 axpby gauss big {numel} offsets {off}")
    else:
        _axpby_case(L, st, "int", 8 * BIG, 0.5, 2.0, (0, 0, 0), "bf16 axpby int big")
        _axpby_case(L, st, "gauss", 8 * BIG, ga, gb, (0, 0, 0), "bf16 axpby gauss big")


# ------------------------------------------------------------------------------------------------------------------- add_n
def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


@pytest.mark.parametrize("st", STORAGES)
def test_add_n(L, BIG, st):
    lib, check = L
    W = R.width(st)
    for numel in (W, 1028 if st == "f32" else 1032, W * BIG):
        for fam in FAMILIES:
            pool = [dev(R.ints((numel,), 120 + j, -3, 3) if fam == "int" else R.gaussian(st, (numel,), 130 + j, 1.0 + j, 0.1 * j)) for j in range(8)]
            bufs = [put(st, row(v)) for v in pool]
            for k in range(1, 9):
                out = out_buf(st, 1, numel)
                check(fn(lib, st, "add_n")(_ptr_array([ptr(b) for b in bufs[:k]]), k, out.ptr, numel, None), "add_n")
                sync()
                what = f"{st} add_n {fam} k {k} numel {numel}"
                guards(out, what=what)
                ref, mag = R.add_n_ref(pool[:k])
                judge(fam, st, out, ref, mag, k - 1, what, "add_n out")
            out = out_buf(st, 1, numel)                         # the same pointer twice
            check(fn(lib, st, "add_n")(_ptr_array([ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[0])]), 3, out.ptr, numel, None), "add_n")
            sync()
            guards(out, what="add_n, a pointer twice")
            judge(fam, st, out, 2 * pool[0] + pool[1], 2 * pool[0].abs() + pool[1].abs(), 2, f"{st} add_n {fam} a pointer twice {numel}", "add_n out")
    out, z = out_buf(st, 1, 64), put(st, row(torch.zeros(72, dtype=F64)))
    P, es, f = ptr(z), esize(st), fn(lib, st, "add_n")
    kfrag = "add_n: 1 <= k <= 8"
    refused(lib, f(_ptr_array([P]), 0, out.ptr, 64, None), ERR_BAD_SHAPE, kfrag, out)
    refused(lib, f(_ptr_array([P] * 9), 9, out.ptr, 64, None), ERR_BAD_SHAPE, kfrag, out)
    if st == "f32":
        refused(lib, f(_ptr_array([P, None]), 2, out.ptr, 64, None), ERR_BAD_SHAPE, "add_n: inputs must be non-null and 16-byte aligned", out)
        refused(lib, f(_ptr_array([P, P + es]), 2, out.ptr, 64, None), ERR_BAD_SHAPE, "add_n: inputs must be non-null and 16-byte aligned", out)
    else:
        refused(lib, f(_ptr_array([P, None]), 2, out.ptr, 64, None), ERR_NULL, "s16_add_n: null input", out)
        refused(lib, f(_ptr_array([P, P + es]), 2, out.ptr, 64, None), ERR_BAD_SHAPE, "input must be 16-byte aligned", out)


# ------------------------------------------------------------------------------------------------------------------ frames
def _frame_shapes(W, BIG):
    return [(n, i * W, None) for n in R.FRAME_N for i in R.FRAME_INNER] + [(3, W * ((BIG + 2) // 3), "p8")]


@pytest.mark.parametrize("st", STORAGES)
def test_add_frames(L, BIG, st):
    lib, check = L
    for n, inner, only in _frame_shapes(R.width(st), BIG):
        for fam in FAMILIES:
            a = R.ints((n, inner), 141, -3, 3) if fam == "int" else R.gaussian(st, (n, inner), 143, 2.0, 0.3)
            b = R.ints((n, inner), 142, -3, 3) if fam == "int" else R.gaussian(st, (n, inner), 144, 1.0, -0.2)
            for pads, (pa, pb, pd) in R.FRAME_PADS3.items():
                if only and pads != only:
                    continue
                ab, bb, dst = put(st, a, inner + pa), put(st, b, inner + pb), out_buf(st, n, inner, inner + pd)
                check(fn(lib, st, "add_frames")(ptr(ab), inner + pa, ptr(bb), inner + pb, dst.ptr, inner + pd, n, inner, None), "add_frames")
                sync()
                what = f"{st} add_frames {fam} n {n} inner {inner} {pads}"
                guards(dst, what=what)
                judge(fam, st, dst, a + b, a.abs() + b.abs(), 1, what, "add_frames dst")


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_copy_frames_and_split(L, BIG):
    lib, check = L
    for n, inner, only in _frame_shapes(4, BIG):
        src = R.gauss32((n, inner), 151, 3.0, 0.2)
        src[0, 0] = -0.0
        for pads, (ps, pd) in R.FRAME_PADS2.items():
            if only and pads != only:
                continue
            sb = put32(src, inner + ps)
            dst, dst2, pk = Guarded(n, inner, inner + pd), Guarded(n, inner, inner + pd), Guarded(n, inner, inner + pd)
            amax = torch.tensor([float(src.abs().max()) * 1.25], dtype=F32, device=DEV)
            want_pk = Guarded(n, inner)
            check(lib.glf_copy_frames(ptr(sb), inner + ps, dst.ptr, inner + pd, n, inner, None), "copy_frames")
            check(lib.glf_copy_frames_split(ptr(sb), inner + ps, dst2.ptr, pk.ptr, inner + pd, n, inner, ptr(amax), None), "copy_frames_split")
            check(lib.glf_split_f16_packed(ptr(sb), n, inner, inner + ps, ptr(amax), want_pk.ptr, inner, None), "split_f16_packed")
            sync()
            what = f"copy_frames n {n} inner {inner} {pads}"
            guards(dst, dst2, pk, want_pk, what=what)
            want = _bits(sb[:, :inner])
            assert torch.equal(_bits(dst.t), want), what + ": copy_frames is not bit-equal to its source"
            assert torch.equal(_bits(dst2.t), want), what + ": copy_frames_split's copy is not bit-equal to its source"
            assert torch.equal(_bits(pk.t), _bits(want_pk.t)), what + ": the packed image differs from glf_split_f16_packed's"
    out, z = Guarded(2, 64, 72), put32(torch.zeros(2, 72, dtype=F64))
    frag = "sizes and strides must be positive multiples of 4"
    refused(lib, lib.glf_copy_frames(ptr(z), 72, out.ptr, 72, 2, 62, None), ERR_BAD_SHAPE, "copy_frames: " + frag, out)
    refused(lib, lib.glf_copy_frames(ptr(z), 70, out.ptr, 72, 2, 64, None), ERR_BAD_SHAPE, "copy_frames: " + frag, out)
    refused(lib, lib.glf_copy_frames(ptr(z) + 4, 72, out.ptr, 72, 2, 64, None), ERR_BAD_SHAPE, "copy_frames: alignment", out)
    refused(lib, lib.glf_add_frames(ptr(z), 72, ptr(z), 72, out.ptr, 70, 2, 64, None), ERR_BAD_SHAPE, "add_frames: " + frag, out)


# ----------------------------------------------------------------------------------------------------------------- dropout
def _dropout_case(L, st, numel, p, seed, step, what):
    lib, check = L
    x = R.dropout_input(st, numel)
    xb, y = put(st, row(x)), out_buf(st, 1, numel)
    ctr = None if step is None else torch.tensor([step], dtype=torch.int64, device=DEV)
    check(fn(lib, st, "dropout")(ptr(xb), y.ptr, numel, p, seed, ptr(ctr), None), "dropout")
    sync()
    guards(y, what=what)                                        # a dropped element is written too: 0 is not the sentinel
    keep = R.dropout_keep(seed, step, numel, p)
    want = R.dropout_ref(x, keep, p)
    exact(y.dense().cpu(), row(want), st == "bf16", what, "dropout y")
    return y.dense().cpu()[0] != 0


@pytest.mark.parametrize("st", STORAGES)
def test_dropout_mask_is_the_restated_hash(L, BIG, st):
    lib, _ = L
    W = 1 if st == "f32" else 8
    for numel in R.DROP_NUMEL + [BIG * W]:
        if numel % W:
            out, z = Guarded16(1, numel + 8), put16(row(torch.zeros(numel + 8, dtype=F64)))
            refused(lib, lib.glf_s16_dropout(ptr(z), out.ptr, numel, 0.5, 1, None, None), ERR_BAD_SHAPE, "s16_dropout: numel must be a positive multiple of 8", out)
            continue
        for seed in R.DROP_SEED:
            for step in R.DROP_STEP:
                for p in R.DROP_P:
                    _dropout_case(L, st, numel, p, seed, step, f"{st} dropout {numel} p {p} seed {seed} step {step}")
    out, z = out_buf(st, 1, 64), put(st, row(torch.zeros(64, dtype=F64)))
    frag = "dropout: numel > 0 and 0 <= p < 1 required" if st == "f32" else "0 <= p < 1"
    refused(lib, fn(lib, st, "dropout")(ptr(z), out.ptr, 64, 1.0, 1, None, None), ERR_BAD_SHAPE, frag, out)
    refused(lib, fn(lib, st, "dropout")(ptr(z), out.ptr, 64, -0.5, 1, None, None), ERR_BAD_SHAPE, frag, out)


def test_dropout_masks_agree_between_storages_and_differ_between_steps(L):
    for seed in R.DROP_SEED:
        k32 = _dropout_case(L, "f32", 264, 0.5, seed, 3, "f32")
        k16 = _dropout_case(L, "bf16", 264, 0.5, seed, 3, "bf16")
        other = _dropout_case(L, "bf16", 264, 0.5, seed, 4, "bf16")
        none = _dropout_case(L, "f32", 264, 0.5, seed, None, "f32")
        zero = _dropout_case(L, "f32", 264, 0.5, seed, 0, "f32")
        assert torch.equal(k32, k16), "the bf16 mask is not the fp32 mask"
        assert not torch.equal(k16, other) and not torch.equal(k32, none), "another step must give another mask"
        assert torch.equal(none, zero), "step 0 is the seed itself"


# ---------------------------------------------------------------------------------------------------------------- max-pool
def _pool_case(L, st, n, h, w, c, kind, what):
    lib, check = L
    dt = F32 if st == "f32" else BF
    x = R.pool_input(n, h, w, c, kind)
    ho, wo = R.pool_out(h), R.pool_out(w)
    yref, code, ind = R.maxpool_ref(x)
    dy = R.ints((n, ho, wo, c), 302, -2, 2)
    dxref = R.maxpool_bwd_ref(dy, ind, h, w)
    xb = x.to(device=DEV, dtype=dt)
    assert R.same_values(xb.double().cpu(), x)
    y, idx, dx = out_buf(st, 1, n * ho * wo * c), Guarded(1, n * ho * wo * c, dtype=torch.uint8), out_buf(st, 1, n * h * w * c)
    dyb, codeb = put(st, row(dy)), dev(code)
    check(fn(lib, st, "maxpool3x3s2_fwd")(ptr(xb), y.ptr, idx.ptr, n, h, w, c, None), "maxpool_fwd")
    check(fn(lib, st, "maxpool3x3s2_bwd")(ptr(dyb), ptr(codeb), dx.ptr, n, h, w, c, None), "maxpool_bwd")
    sync()
    guards(y, idx, dx, what=what)
    assert R.same_values(y.f64().cpu().view(yref.shape), yref), what + ": pooled values differ from F.max_pool2d"
    bad = (idx.t.cpu().view(code.shape) != code).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} window codes differ from ATen's; first at {bad[0].tolist()}: got {int(idx.t.cpu().view(code.shape)[tuple(bad[0])])}, want {int(code[tuple(bad[0])])}"
    bf16_holds(dxref)
    exact(dx.dense(), dev(row(dxref)), st == "bf16", what + " dx", "maxpool dx")


@pytest.mark.parametrize("kind", ["plain", "relu", "special"])
@pytest.mark.parametrize("st", STORAGES)
def test_maxpool_values_indices_routing(L, st, kind):
    for n, h, w in R.POOL_SHAPES:
        for c in R.POOL_C:
            if st == "bf16" and c % 8:
                continue
            _pool_case(L, st, n, h, w, c, kind, f"{st} maxpool {kind} {n} x {h} x {w} x {c}")


@pytest.mark.parametrize("st", STORAGES)
def test_maxpool_second_trip(L, st):
    n, h, w = R.POOL_BIG
    _pool_case(L, st, n, h, w, 256 if st == "f32" else 512, "plain", f"{st} maxpool big")


def test_maxpool_refusals(L):
    lib, _ = L
    f32o, b16o, idx = Guarded(1, 4096), Guarded16(1, 4096), Guarded(1, 4096, dtype=torch.uint8)
    z32, z16, zi = put32(row(torch.zeros(4096, dtype=F64))), put16(row(torch.zeros(4096, dtype=F64))), torch.zeros(4096, dtype=torch.uint8, device=DEV)
    bufs = (f32o, b16o, idx)
    n, h, w = 1, 5, 5
    for c in (1, 6):
        refused(lib, lib.glf_maxpool3x3s2_fwd(ptr(z32), f32o.ptr, idx.ptr, n, h, w, c, None), ERR_BAD_SHAPE, "maxpool_fwd: bad shape", *bufs)
        refused(lib, lib.glf_maxpool3x3s2_bwd(ptr(z32), ptr(zi), f32o.ptr, n, h, w, c, None), ERR_BAD_SHAPE, "maxpool_bwd: bad shape", *bufs)
    for c in (4, 12):
        refused(lib, lib.glf_s16_maxpool3x3s2_fwd(ptr(z16), b16o.ptr, idx.ptr, n, h, w, c, None), ERR_BAD_SHAPE, "channel count must be a positive multiple of 8", *bufs)
        refused(lib, lib.glf_s16_maxpool3x3s2_bwd(ptr(z16), ptr(zi), b16o.ptr, n, h, w, c, None), ERR_BAD_SHAPE, "channel count must be a positive multiple of 8", *bufs)
    # idx is read and written one pixel's channel group at a time: 4 bytes (fp32), 8 bytes (bf16)
    for off in (1, 2, 3):
        refused(lib, lib.glf_maxpool3x3s2_fwd(ptr(z32), f32o.ptr, idx.ptr + off, n, h, w, 8, None), ERR_BAD_SHAPE, "maxpool_fwd: alignment", *bufs)
        refused(lib, lib.glf_maxpool3x3s2_bwd(ptr(z32), ptr(zi) + off, f32o.ptr, n, h, w, 8, None), ERR_BAD_SHAPE, "maxpool_bwd: alignment", *bufs)
    for off in (1, 2, 4, 6):
        refused(lib, lib.glf_s16_maxpool3x3s2_fwd(ptr(z16), b16o.ptr, idx.ptr + off, n, h, w, 8, None), ERR_BAD_SHAPE, "s16_maxpool_fwd: idx must be 8-byte aligned", *bufs)
        refused(lib, lib.glf_s16_maxpool3x3s2_bwd(ptr(z16), ptr(zi) + off, b16o.ptr, n, h, w, 8, None), ERR_BAD_SHAPE, "s16_maxpool_bwd: idx must be 8-byte aligned", *bufs)
    refused(lib, lib.glf_maxpool3x3s2_fwd(ptr(z32) + 4, f32o.ptr, idx.ptr, n, h, w, 8, None), ERR_BAD_SHAPE, "maxpool_fwd: alignment", *bufs)
    refused(lib, lib.glf_s16_maxpool3x3s2_bwd(ptr(z16), ptr(zi), b16o.ptr + 2, n, h, w, 8, None), ERR_BAD_SHAPE, "dx must be 16-byte aligned", *bufs)


# -------------------------------------------------------------------------------------------------------------------- gate
def _gate_data(st, fam, rows, c, seed):
    if fam == "int":
        return R.ints((rows, c), seed, -3, 3), R.ints((rows, c), seed + 1, -2, 2)
    return R.gaussian(st, (rows, c), seed, 2.0, 0.3), R.gaussian(st, (rows, c), seed + 1, 1.0, 0.1)


@pytest.mark.parametrize("st,c", [(st, c) for st in STORAGES for c in R.GATE_C[st]])
def test_gate_fwd_bwd(L, st, c):
    """lane 0 alone (c = 4 / 8), exactly 64 lanes (256 / 512 would be: 2048 makes 8 / 4 trips), 64 + 1 (264 fp32 -> 66 accesses)"""
    lib, check = L
    w = R.GATE_WEIGHT
    for rows in R.GATE_ROWS:
        for ncls in R.GATE_NCLS:
            cls, ctr = R.gate_inputs(rows, ncls)
            assert R.gate_conditions(cls)
            bi, a_ref, ka = R.gate_fwd_ref(cls, ctr, w)
            clsb, ctrb = vec32(cls), vec32(ctr)
            for fam in FAMILIES:
                f, dy = _gate_data(st, fam, rows, c, 511)
                what = f"{st} gate {fam} rows {rows} ncls {ncls} c {c}"
                fb, dyb = put(st, f), put(st, dy)
                y, a, am = out_buf(st, rows, c), Guarded(1, rows), Guarded(1, rows, dtype=torch.int32)
                check(fn(lib, st, "gate_fwd")(ptr(clsb), ncls, ptr(ctrb), ptr(fb), y.ptr, a.ptr, am.ptr, w, rows, c, None), "gate_fwd")
                sync()
                guards(y, a, am, what=what)
                assert torch.equal(am.t[0].cpu(), bi), what + ": argmax is not the first maximum"
                gate_rel(a.f64()[0].cpu(), a_ref, ka, False, what + " a", "gate a")
                a_got = a.f64()[0].cpu()
                exact(y.dense().cpu(), R.product32(f, a_got[:, None]), st == "bf16", what + " y", "gate y")
                # backward with a given a (the float64 one rounded to fp32) and the reference's argmax
                a_in = a_ref.float().double()
                df, dcls, dctr = out_buf(st, rows, c), Guarded(rows, ncls), Guarded(1, rows)
                a_inb, bib = vec32(a_in), dev(bi)
                check(fn(lib, st, "gate_bwd")(ptr(dyb), ptr(fb), ptr(clsb), ncls, ptr(ctrb), ptr(a_inb), ptr(bib), w, df.ptr, dcls.ptr,
                                              dctr.ptr, rows, c, None), "gate_bwd")
                sync()
                guards(df, dcls, dctr, what=what + " bwd")
                exact(df.dense().cpu(), R.product32(dy, a_in[:, None]), st == "bf16", what + " df", "gate df")
                b = R.gate_bwd_ref(dy, f, cls, ctr, a_in, bi, w)
                kda = R.k_gate_da(st, c, fam)
                got = dcls.f64().cpu()
                assert bool((got[~b.hot] == 0).all()), what + ": dcls off the argmax column is not exactly zero"
                gate(got[b.hot], b.dcls[b.hot], b.dclsm[b.hot] * (kda + b.kcls + 4.0) / 4.0, 0, False, what + " dcls", "gate dcls")
                gate(dctr.f64()[0].cpu(), b.dctr, b.dctrm * (kda + b.kctr + 4.0) / 4.0, 0, False, what + " dctr", "gate dctr")


def test_gate_refusals(L):
    lib, _ = L
    o32, o16, of = Guarded(4, 64), Guarded16(4, 64), Guarded(1, 64)
    z32, z16 = put32(torch.zeros(4, 72, dtype=F64)), put16(torch.zeros(4, 72, dtype=F64))
    v = torch.zeros(64, dtype=F32, device=DEV)
    vi = torch.zeros(64, dtype=torch.int32, device=DEV)
    bufs = (o32, o16, of)
    refused(lib, lib.glf_gate_fwd(ptr(v), 2, ptr(v), ptr(z32), o32.ptr, of.ptr, ptr(vi), 1.0, 4, 6, None), ERR_BAD_SHAPE, "gate_fwd: bad shape", *bufs)
    refused(lib, lib.glf_gate_fwd(ptr(v), 2, ptr(v), ptr(z32) + 4, o32.ptr, of.ptr, ptr(vi), 1.0, 4, 8, None), ERR_BAD_SHAPE, "gate_fwd: alignment", *bufs)
    refused(lib, lib.glf_s16_gate_fwd(ptr(v), 2, ptr(v), ptr(z16), o16.ptr, of.ptr, ptr(vi), 1.0, 4, 12, None), ERR_BAD_SHAPE, "channel count must be a positive multiple of 8", *bufs)
    refused(lib, lib.glf_gate_bwd(ptr(z32), ptr(z32), ptr(v), 2, ptr(v), ptr(v), ptr(vi), 1.0, o32.ptr, of.ptr, of.ptr + 128, 4, 6, None), ERR_BAD_SHAPE, "gate_bwd: bad shape", *bufs)
    refused(lib, lib.glf_s16_gate_bwd(ptr(z16), ptr(z16), ptr(v), 2, ptr(v), ptr(v), ptr(vi), 1.0, o16.ptr + 2, of.ptr, of.ptr + 128, 4, 8, None), ERR_BAD_SHAPE, "df must be 16-byte aligned", *bufs)


# ------------------------------------------------------------------------------------------------ row sums and broadcasts
def _rows_x(fam, n, p, c, seed=521):
    return R.ints((n * p, c), seed, -3, 3) if fam == "int" else R.gauss32((n * p, c), seed + 1, 2.0, 0.7)


@pytest.mark.parametrize("c", R.ROWS_C)
def test_sum_rows_and_avgpool(L, c):
    """Which kernel a case reaches (pointwise_ref.sum_rows_uses_double): c in {4, 60, 64, 68, 260} with ld = c or c + 4 and an
    aligned base -> sum_rows4_kernel (16-byte loads, double sums); c in {1, 3}, ld = c + 1, or the base off by one element ->
    sum_rows_kernel (scalar loads, fp32 sums)."""
    lib, check = L
    for n in R.ROWS_N:
        for p in R.ROWS_P:
            for fam in FAMILIES:
                x = _rows_x(fam, n, p, c)
                for which, base_off in (("c", 0), ("cw", 0), ("c1", 0), ("c", 1), ("avg", 0)):
                    avg = which == "avg"
                    ld = c if avg else R.rows_ld(c, which)
                    scale = float(np.float32(1.0) / np.float32(p)) if avg else 0.5
                    if avg and fam == "int" and p & (p - 1):
                        continue                                # 1 / p is dyadic only for powers of two
                    xb = put32(x, ld)
                    flat = torch.full((n * p * ld + 4,), float("nan"), dtype=F32, device=DEV)
                    flat[base_off:base_off + n * p * ld] = xb.view(-1)
                    y = Guarded(n, c)
                    if avg:
                        check(lib.glf_avgpool_fwd(ptr(flat), y.ptr, n, p, c, None), "avgpool_fwd")
                    else:
                        check(lib.glf_sum_rows_fwd(ptr(flat) + 4 * base_off, ld, y.ptr, scale, n, p, c, None), "sum_rows_fwd")
                    sync()
                    what = f"sum_rows {fam} n {n} p {p} c {c} ld {ld} base offset {base_off} {'avgpool' if avg else ''}"
                    guards(y, what=what)
                    ref, mag = R.sum_rows_ref(x, n, p, scale)
                    dbl = R.sum_rows_uses_double(c, ld, base_off)
                    if fam == "int":
                        R.assert_exact(2 * mag)
                        exact(y.dense(), dev(ref), False, what, "sum_rows y, double sums" if dbl else "sum_rows y, fp32 sums")
                    else:
                        gate(y.f64(), dev(ref), dev(mag), R.k_sum_rows(p, dbl), False, what, "sum_rows y, double sums" if dbl else "sum_rows y, fp32 sums")


def _bcast_case(L, fam, n, p, c, ld, base_off, entry, what):
    lib, check = L
    x = R.ints((n, c), 531, -3, 3) if fam == "int" else R.gauss32((n, c), 532, 2.0, 0.7)
    scale = 1.0 if entry == "fwd" else 0.5
    xb = torch.full((n * c + 4,), float("nan"), dtype=F32, device=DEV)
    xb[base_off:base_off + n * c] = dev(x).float().view(-1)
    y = Guarded(n * p, c, ld)
    y0 = None
    if entry == "add":
        y0 = R.ints((n * p, c), 533, -2, 2) if fam == "int" else R.gauss32((n * p, c), 534, 1.0, -0.4)
        y.fill(dev(y0))
        check(lib.glf_bcast_rows_add(ptr(xb) + 4 * base_off, y.ptr, ld, scale, n, p, c, None), "bcast_rows_add")
    elif entry == "fwd":
        check(lib.glf_bcast_rows_fwd(ptr(xb) + 4 * base_off, y.ptr, ld, n, p, c, None), "bcast_rows_fwd")
    else:
        check(lib.glf_bcast_rows_scaled(ptr(xb) + 4 * base_off, y.ptr, ld, scale, n, p, c, None), "bcast_rows_scaled")
    sync()
    guards(y, what=what)
    ref, mag = R.bcast_ref(x, p, scale, y0)
    judge(fam, "f32", y, ref, mag, R.K_BCAST_ADD if entry == "add" else R.K_BCAST, what, "bcast_rows_add y" if entry == "add" else "bcast_rows y")


@pytest.mark.parametrize("c", R.ROWS_C)
def test_bcast_rows_fp32(L, c):
    """float4 stores iff c % 4 == 0, ld % 4 == 0 and both pointers on 16 bytes (c in {4, 60, 64, 68, 260} with ld = c or c + 4);
    single elements otherwise (c in {1, 3}, ld = c + 1, x off by one element).  _add takes the float4 form only."""
    lib, _ = L
    for n in R.ROWS_N:
        for p in R.ROWS_P:
            for fam in FAMILIES:
                for which, base_off in (("c", 0), ("cw", 0), ("c1", 0), ("c", 1)):
                    ld = R.rows_ld(c, which)
                    for entry in ("scaled", "fwd", "add"):
                        what = f"bcast_rows_{entry} {fam} n {n} p {p} c {c} ld {ld} base offset {base_off}"
                        if entry == "add" and not (c % 4 == 0 and ld % 4 == 0 and base_off == 0):
                            if fam == "int" and n == 1 and p == 1:
                                y, z = Guarded(4, c, ld), torch.zeros(c + 4, dtype=F32, device=DEV)
                                refused(lib, lib.glf_bcast_rows_add(ptr(z) + 4 * base_off, y.ptr, ld, 0.5, 1, 4, c, None), ERR_UNSUPPORTED,
                                        "bcast_rows_add: c and ldy must be multiples of 4", y)
                            continue
                        _bcast_case(L, fam, n, p, c, ld, base_off, entry, what)


def test_bcast_rows_second_trip(L, BIG):
    n, p = 3, 196
    q = (BIG + n * p - 1) // (n * p)                             # accesses per row
    for entry, c, ld in (("scaled", 4 * q, 4 * q + 4), ("scaled", q, q), ("add", 4 * q, 4 * q + 4)):
        _bcast_case(L, "int", n, p, c, ld, 0, entry, f"bcast_rows_{entry} big c {c}")
    _s16_bcast_case(L, "int", n, p, 8 * q, 8 * q + 8, DT_F32, "s16_bcast_rows big")


def _s16_bcast_case(L, fam, n, p, c, ld, x_dtype, what):
    lib, check = L
    x = R.ints((n, c), 541, -3, 3) if fam == "int" else (R.gauss32 if x_dtype == DT_F32 else R.gauss)((n, c), 542, 2.0, 0.7)
    xb = put32(x) if x_dtype == DT_F32 else put16(x)
    y = Guarded16(n * p, c, ld)
    check(lib.glf_s16_bcast_rows(ptr(xb), x_dtype, y.ptr, ld, 0.5, n, p, c, None), "s16_bcast_rows")
    sync()
    guards(y, what=what)
    ref, mag = R.bcast_ref(x, p, 0.5)
    judge(fam, "bf16", y, ref, mag, R.K_BCAST, what, "s16_bcast_rows y")


@pytest.mark.parametrize("c", R.ROWS_C16)
def test_s16_bcast_rows(L, c):
    for n in R.ROWS_N:
        for p in R.ROWS_P:
            for fam in FAMILIES:
                for ld in (c, c + 8):
                    for dt in (DT_F32, DT_BF16):
                        _s16_bcast_case(L, fam, n, p, c, ld, dt, f"s16_bcast_rows {fam} n {n} p {p} c {c} ld {ld} x {'fp32' if dt == DT_F32 else 'bf16'}")


def test_rows_refusals(L):
    lib, _ = L
    y, y16 = Guarded(4, 64), Guarded16(4, 64)
    z, z16 = torch.zeros(4096, dtype=F32, device=DEV), put16(torch.zeros(4, 72, dtype=F64))
    refused(lib, lib.glf_sum_rows_fwd(ptr(z), 8, y.ptr, 1.0, 65536, 1, 8, None), ERR_BAD_SHAPE, "sum_rows: bad shape", y, y16)
    refused(lib, lib.glf_sum_rows_fwd(ptr(z), 7, y.ptr, 1.0, 2, 4, 8, None), ERR_BAD_SHAPE, "sum_rows: bad shape", y, y16)
    refused(lib, lib.glf_bcast_rows_scaled(ptr(z), y.ptr, 7, 1.0, 2, 2, 8, None), ERR_BAD_SHAPE, "bcast_rows: bad shape", y, y16)
    refused(lib, lib.glf_bcast_rows_add(ptr(z), y.ptr, 7, 1.0, 2, 2, 8, None), ERR_BAD_SHAPE, "bcast_rows_add: bad shape", y, y16)
    refused(lib, lib.glf_bcast_rows_add(ptr(z), y.ptr, 8, 1.0, 2, 2, 6, None), ERR_UNSUPPORTED, "bcast_rows_add: c and ldy must be multiples of 4", y, y16)
    refused(lib, lib.glf_s16_bcast_rows(ptr(z), DT_F32, y16.ptr, 16, 1.0, 2, 2, 12, None), ERR_BAD_SHAPE, "channel count must be a positive multiple of 8", y, y16)
    refused(lib, lib.glf_s16_bcast_rows(ptr(z), DT_F32, y16.ptr, 12, 1.0, 2, 2, 8, None), ERR_BAD_SHAPE, "ldy must be a multiple of 8", y, y16)
    refused(lib, lib.glf_s16_bcast_rows(ptr(z), 7, y16.ptr, 8, 1.0, 2, 2, 8, None), ERR_UNSUPPORTED, "s16_bcast_rows: x_dtype", y, y16)


# ----------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("cols", R.SOFT_COLS)
def test_softmax_rows(L, cols):
    lib, check = L
    for rows in R.SOFT_ROWS:
        x = R.softmax_input(rows, cols)
        pref, kel = R.softmax_ref(x)
        for pad in R.SOFT_PAD:
            ld = cols + pad
            buf = Guarded(rows, ld)
            buf.t[:, :cols] = dev(x).float()
            if pad:
                check(lib.glf_softmax_rows_ld(buf.ptr, rows, cols, ld, None), "softmax_rows_ld")
            else:
                check(lib.glf_softmax_rows(buf.ptr, rows, cols, None), "softmax_rows")
            sync()
            what = f"softmax rows {rows} cols {cols} ld {ld}"
            guards(buf, what=what)
            assert bool((buf.t[:, cols:] == 0).all()), what + ": the columns cols .. ld must read exactly 0"
            gate_rel(buf.f64()[:, :cols], dev(pref), dev(kel), False, what, "softmax p", extra=torch.full_like(dev(pref), R.TINY))
            gate_rel(buf.f64()[:, :cols], dev(pref), dev(kel), False, what, "softmax p, p >= 2^-100", sure=dev(pref) >= 2.0 ** -100)
            for fam in FAMILIES:
                p, dy = R.softmax_bwd_inputs(fam, rows, cols)
                pb, dp = put32(p, ld), Guarded(rows, ld)
                dp.t[:, :cols] = dev(dy).float()
                if pad:
                    check(lib.glf_softmax_rows_bwd_ld(ptr(pb), dp.ptr, rows, cols, ld, None), "softmax_rows_bwd_ld")
                else:
                    check(lib.glf_softmax_rows_bwd(ptr(pb), dp.ptr, rows, cols, None), "softmax_rows_bwd")
                sync()
                guards(dp, what=what + " bwd")
                assert bool((dp.t[:, cols:] == 0).all()), what + " bwd: the columns cols .. ld must read exactly 0"
                ref, mag = R.softmax_bwd_ref(p, dy)
                got = Guarded(rows, cols).fill(dp.t[:, :cols])
                judge(fam, "f32", got, ref, mag, R.k_softmax_bwd(cols), what + f" bwd {fam}", "softmax_bwd dp")
    buf = Guarded(2, 8)
    refused(lib, lib.glf_softmax_rows_ld(buf.ptr, 2, 8, 7, None), ERR_BAD_SHAPE, "softmax_rows_ld: bad shape", buf)
    refused(lib, lib.glf_softmax_rows_bwd_ld(buf.ptr, buf.ptr, 2, 8, 7, None), ERR_BAD_SHAPE, "softmax_rows_bwd_ld: bad shape", buf)
    refused(lib, lib.glf_softmax_rows(buf.ptr, 0, 8, None), ERR_BAD_SHAPE, "softmax_rows: bad shape", buf)


# ---------------------------------------------------------------------------------------------------------------- bilinear
def _bilinear_case(L, fam, n, h, w, c, ho, wo, what, fwd=True, bwd=True):
    lib, check = L
    if fwd:
        x = R.ints((n, h, w, c), 551, -3, 3) if fam == "int" else R.gauss32((n, h, w, c), 552, 2.0, 0.5)
        xb, y = put32(row(x)), Guarded(1, n * c * ho * wo)
        check(lib.glf_bilinear_up_fwd(ptr(xb), y.ptr, n, h, w, c, ho, wo, None), "bilinear_up_fwd")
        sync()
        guards(y, what=what)
        ref, mag = R.bilinear_fwd_ref(x, ho, wo)
        gate(y.f64(), dev(row(ref)), dev(row(mag)), R.k_bilinear_fwd(h, w), False, what + " fwd", "bilinear y")
        if (h, w) == (ho, wo):
            exact(y.dense(), dev(row(x.permute(0, 3, 1, 2))), False, what + " identity", "bilinear y")
    if bwd:
        dy = R.ints((n, c, ho, wo), 553, -2, 2) if fam == "int" else R.gauss32((n, c, ho, wo), 554, 1.0, 0.2)
        dyb, dx = put32(row(dy)), Guarded(1, n * h * w * c)
        check(lib.glf_bilinear_up_bwd(ptr(dyb), dx.ptr, n, h, w, c, ho, wo, None), "bilinear_up_bwd")
        sync()
        guards(dx, what=what)
        ref, mag, rc, cc = R.bilinear_bwd_ref(dy, h, w)
        gate(dx.f64(), dev(row(ref)), dev(row(mag)), R.k_bilinear_bwd(h, w, rc, cc), False, what + " bwd", "bilinear dx")
        if (h, w) == (ho, wo):
            exact(dx.dense(), dev(row(dy.permute(0, 2, 3, 1))), False, what + " identity bwd", "bilinear dx")


@pytest.mark.parametrize("shape", R.BIL_SHAPES)
def test_bilinear_up(L, shape):
    h, w, ho, wo = shape
    for n in R.BIL_N:
        for c in R.BIL_C:
            for fam in FAMILIES:
                _bilinear_case(L, fam, n, h, w, c, ho, wo, f"bilinear {fam} n {n} c {c} {h} x {w} -> {ho} x {wo}")


def test_bilinear_second_trip_and_refusals(L, BIG):
    lib, _ = L
    side = math.isqrt(BIG) + 1
    _bilinear_case(L, "gauss", 1, 5, 7, 1, side, side, f"bilinear big fwd -> {side} x {side}", bwd=False)
    hs = math.isqrt((BIG + 3) // 4) + 1
    _bilinear_case(L, "gauss", 1, hs, hs, 4, hs + 37, hs + 17, f"bilinear big bwd {hs} x {hs} x 4", fwd=False)
    out, z = Guarded(1, 256), torch.zeros(256, dtype=F32, device=DEV)
    refused(lib, lib.glf_bilinear_up_bwd(ptr(z), out.ptr, 1, 4, 4, 1, 3, 8, None), ERR_BAD_SHAPE, "bilinear_up_bwd: up-sampling only", out)
    refused(lib, lib.glf_bilinear_up_bwd(ptr(z), out.ptr, 1, 4, 4, 1, 8, 3, None), ERR_BAD_SHAPE, "bilinear_up_bwd: up-sampling only", out)
    refused(lib, lib.glf_bilinear_up_fwd(ptr(z), out.ptr, 1, 4, 4, 0, 8, 8, None), ERR_BAD_SHAPE, "bilinear_up_fwd: bad shape", out)


# ------------------------------------------------------------------------------------------------------------ BCE, overlap
def test_bce_and_overlap_counts(L, BIG):
    lib, check = L
    for numel in R.BCE_NUMEL + [BIG]:
        x, t = R.bce_inputs(numel)
        assert R.overlap_condition(x)
        xb, tb = put32(row(x)), put32(row(t))
        counts = Guarded(1, 4, dtype=torch.int64)
        check(lib.glf_overlap_counts(ptr(xb), ptr(tb), counts.ptr, numel, None), "overlap_counts")
        sync()
        guards(counts, what=f"overlap {numel}")
        assert torch.equal(counts.t[0].cpu(), R.overlap_ref(x, t)), f"overlap_counts {numel}: {counts.t[0].tolist()} != {R.overlap_ref(x, t).tolist()}"
        for want_dx in (False, True):
            for gdev in (None, 0.25):
                gs = 1.0 / 64
                g = gs * (gdev or 1.0)
                loss, dx = Guarded(1, 1, dtype=F64), Guarded(1, numel) if want_dx else None
                gsd = None if gdev is None else torch.tensor([gdev], dtype=F32, device=DEV)
                check(lib.glf_bce_logits_sum(ptr(xb), ptr(tb), loss.ptr, ptr(dx), gs, ptr(gsd), numel, None), "bce_logits_sum")
                sync()
                what = f"bce {numel} dx {want_dx} grad_scale_dev {gdev}"
                guards(loss, dx, what=what)
                lref, lmag, dref, dmag = R.bce_ref(dev(x), dev(t), g)
                gate(loss.f64(), lref.view(1, 1), lmag.view(1, 1), R.K_BCE, False, what + " loss", "bce loss")
                if want_dx:
                    gate(dx.f64(), row(dref), row(dmag), R.K_BCE_DX, False, what + " dx", "bce dx", extra=torch.full_like(row(dmag), R.TINY * abs(g)))
                    gate(dx.f64(), row(dref), row(dmag), R.K_BCE_DX, False, what + " dx", "bce dx, |x| <= 80", sure=row(dev(x)).abs() <= 80)
    out = Guarded(1, 8, dtype=F64)
    z = torch.zeros(8, dtype=F32, device=DEV)
    refused(lib, lib.glf_bce_logits_sum(ptr(z), ptr(z), out.ptr, None, 1.0, None, 0, None), ERR_BAD_SHAPE, "bce_logits_sum: numel must be > 0", out)
    refused(lib, lib.glf_bce_logits_sum(ptr(z), None, out.ptr, None, 1.0, None, 8, None), ERR_NULL, "bce_logits_sum: null argument", out)
    refused(lib, lib.glf_overlap_counts(ptr(z), ptr(z), None, 8, None), ERR_NULL, "overlap_counts: null argument", out)


# -------------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("shape", R.STEM_SHAPES)
def test_stem7x7(L, shape):
    """ho, wo = 1 (7, 7, 0 and 1, 1, 3), 16, 17 x 32, 18 x 33, 12 x 9: one, two and ragged 16 x 16 conv tiles; pooled 1 .. 17: one,
    two, three 7 x 7 pool tiles, ragged"""
    lib, check = L
    h, w, pad = shape
    for n in R.STEM_N:
        for fam in FAMILIES:
            I = R.stem_inputs(fam, n, h, w, pad)
            ho, wo = I.ho, I.wo
            what = f"stem {fam} n {n} {h} x {w} pad {pad}"
            xb, wb, bb = put32(row(I.x)), put32(row(I.w)), vec32(I.bias)
            yref, ymag = R.stem_fwd_ref(I.x, I.w, I.bias, pad)
            y0ref, y0mag = R.stem_fwd_ref(I.x, I.w, torch.zeros(64, dtype=F64), pad)
            for st in STORAGES:
                for bias in (True, False):
                    y = out_buf(st, 1, n * ho * wo * 64)
                    check(fn(lib, st, "stem7x7_fwd")(ptr(xb), ptr(wb), ptr(bb) if bias else None, y.ptr, n, h, w, 64, pad, None), "stem7x7_fwd")
                    sync()
                    guards(y, what=what)
                    judge(fam, st, y, yref if bias else y0ref, ymag if bias else y0mag, R.K_STEM_FWD, f"{what} {st} fwd bias {bias}", "stem y")
                dyb = put(st, row(I.dy))
                nws = lib.glf_stem7x7_wgrad_workspace(n, h, w, 64, pad)
                ws = Guarded(1, nws)
                dw, db = Guarded(1, 64 * 49), Guarded(1, 64)
                check(fn(lib, st, "stem7x7_wgrad")(ptr(xb), ptr(dyb), dw.ptr, db.ptr, ws.ptr, n, h, w, 64, pad, None), "stem7x7_wgrad")
                sync()
                guards(dw, db, ws, what=what + " wgrad")
                dwref, dwmag, dbref, dbmag = R.stem_wgrad_ref(I.x, I.dy, pad)
                k = R.k_stem_wgrad(ho, wo)
                judge(fam, "f32", dw, dwref, dwmag, k, f"{what} {st} dw", "stem dw")
                judge(fam, "f32", db, dbref, dbmag, k, f"{what} {st} db", "stem db")
            hp, wp = (ho - 1) // 2 + 1, (wo - 1) // 2 + 1
            pref, pmag = R.stem_pool_ref(yref, ymag, I.mean, I.invstd, I.gamma, I.beta)
            mb, ib, gb, eb = vec32(I.mean), vec32(I.invstd), vec32(I.gamma), vec32(I.beta)
            for start in (None, 0.0, 1.0e6):
                yp = Guarded(1, n * hp * wp * 64)
                amax = None if start is None else Guarded(1, 1).fill(torch.tensor([[start]]))
                check(lib.glf_stem7x7_bn_relu_pool(ptr(xb), ptr(wb), ptr(bb), ptr(mb), ptr(ib), ptr(gb), ptr(eb),
                                                   yp.ptr, n, h, w, 64, pad, ptr(amax), None), "stem7x7_bn_relu_pool")
                sync()
                guards(yp, what=what + " pool")
                judge(fam, "f32", yp, pref, pmag, R.K_STEM_POOL, what + " pool", "stem pool y")
                if amax is not None:
                    assert amax.intact()
                    assert float(amax.t) == max(start, float(yp.t.max())), what + ": amax_out is not max(what was there, what was written)"


def test_stem_refusals(L):
    lib, _ = L
    y, y16 = Guarded(1, 4096), Guarded16(1, 4096)
    z = torch.zeros(4096, dtype=F32, device=DEV)
    Z = ptr(z)
    for st, o in (("f32", y), ("bf16", y16)):
        f = fn(lib, st, "stem7x7_fwd")
        refused(lib, f(Z, Z, Z, o.ptr, 1, 8, 8, 32, 0, None), ERR_UNSUPPORTED, "stem7x7: Cout must be 64", y, y16)
        refused(lib, f(Z, Z, Z, o.ptr, 1, 8, 8, 64, 4, None), ERR_BAD_SHAPE, "stem7x7_fwd: bad shape", y, y16)
        refused(lib, f(Z, Z, Z, o.ptr + 4, 1, 8, 8, 64, 0, None), ERR_BAD_SHAPE, "stem7x7_fwd: y must be 16-byte aligned", y, y16)
        g = fn(lib, st, "stem7x7_wgrad")
        refused(lib, g(Z, Z, y.ptr, None, y.ptr + 4096, 1, 8, 8, 32, 0, None), ERR_UNSUPPORTED, "stem7x7: Cout must be 64", y, y16)
        refused(lib, g(Z, Z, y.ptr, None, y.ptr + 4096, 1, 8, 8, 64, 4, None), ERR_BAD_SHAPE, "stem7x7_wgrad: bad shape", y, y16)
    p = lambda cout=64, pad=0, off=0: lib.glf_stem7x7_bn_relu_pool(Z, Z, Z, Z, Z, Z, Z, y.ptr + off, 1, 8, 8, cout, pad, None, None)
    refused(lib, p(cout=32), ERR_UNSUPPORTED, "stem7x7: Cout must be 64", y, y16)
    refused(lib, p(pad=4), ERR_BAD_SHAPE, "stem7x7_bn_relu_pool: bad shape", y, y16)
    refused(lib, p(off=4), ERR_BAD_SHAPE, "stem7x7_bn_relu_pool: y must be 16-byte aligned", y, y16)


# --------------------------------------------------------------------------------------------- transposes and re-layouts
def _tr_source(st, batch, rows, cols, seed=561):
    """distinct values per element where the format allows: a permutation shows as a difference"""
    v = (torch.arange(batch * rows * cols, dtype=F64) % 251) - 125.0 if st == "bf16" else torch.arange(batch * rows * cols, dtype=F64) - 7.0
    return v.view(batch, rows, cols)


@pytest.mark.parametrize("st", STORAGES)
def test_transpose2d(L, st):
    lib, check = L
    dt = F32 if st == "f32" else torch.int16
    dims, tile = R.TR_DIMS[st], R.TR_TILE[st]
    for batch in R.TR_BATCH:
        for rows in dims:
            for cols in dims:
                src = _tr_source(st, batch, rows, cols)
                sb = put(st, src.view(batch * rows, cols))
                dst = out_buf(st, batch * cols, rows)
                check(fn(lib, st, "transpose2d")(ptr(sb), dst.ptr, rows, cols, batch, None), "transpose2d")
                sync()
                what = f"{st} transpose2d batch {batch} {rows} x {cols}"
                guards(dst, what=what)
                exact(dst.dense(), dev(src.transpose(1, 2).reshape(batch * cols, rows)), st == "bf16", what, "transpose2d")
                for rows_pad in R.rows_pads(rows, tile):
                    for ps, pd in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        ld_s, ld_d = cols + 3 * ps, rows_pad + 3 * pd
                        bs_s, bs_d = rows * ld_s + 5 * ps, cols * ld_d + 5 * pd
                        slive, soff = R.strided_live(batch, rows, cols, ld_s, bs_s)
                        sflat = torch.full((slive.numel(),), float("nan"), dtype=F64)
                        sflat[soff] = src.reshape(-1)
                        sbuf = sflat.to(device=DEV, dtype=F32 if st == "f32" else BF)
                        dlive, doff = R.strided_live(batch, cols, rows_pad, ld_d, bs_d)
                        out = GuardedMask(dlive, dtype=dt)
                        check(fn(lib, st, "transpose2d_strided")(ptr(sbuf), ld_s, bs_s, out.ptr, ld_d, bs_d, rows, cols, rows_pad, batch, None), "transpose2d_strided")
                        sync()
                        what2 = f"{what} strided rows_pad {rows_pad} pads src {ps} dst {pd}"
                        guards(out, what=what2)
                        want = torch.zeros(batch, cols, rows_pad, dtype=F64)
                        want[:, :, :rows] = src.transpose(1, 2)
                        got = out.body[dev(doff)]
                        got = got.view(BF) if st == "bf16" else got
                        exact(got, dev(want.reshape(-1)), st == "bf16", what2, "transpose2d_strided")
    out, z = out_buf(st, 8, 8), put(st, torch.zeros(8, 8, dtype=F64))
    f = fn(lib, st, "transpose2d_strided")
    refused(lib, f(ptr(z), 7, 64, out.ptr, 8, 64, 8, 8, 8, 1, None), ERR_BAD_SHAPE, "transpose2d_strided: bad shape", out)
    refused(lib, f(ptr(z), 8, 64, out.ptr, 8, 64, 8, 8, 9, 1, None), ERR_BAD_SHAPE, "transpose2d_strided: bad shape", out)
    refused(lib, f(ptr(z), 8, 64, out.ptr, 8, 64, 8, 8, 7, 1, None), ERR_BAD_SHAPE, "transpose2d_strided: bad shape", out)
    refused(lib, fn(lib, st, "transpose2d")(ptr(z), out.ptr, 8, 0, 1, None), ERR_BAD_SHAPE, "transpose2d: bad", out)


@pytest.mark.parametrize("cout,cin,taps", R.RELAYOUT)
def test_weight_relayouts(L, cout, cin, taps):
    lib, check = L
    n = cout * cin * taps
    w = R.gauss32((cout, cin, taps), 571)
    wb = put32(row(w))
    tm, tmt, back = Guarded(1, n), Guarded(1, n), Guarded(1, n)
    check(lib.glf_oihw_to_tap_major(ptr(wb), tm.ptr, cout, cin, taps, None), "oihw_to_tap_major")
    check(lib.glf_oihw_to_tap_major_t(ptr(wb), tmt.ptr, cout, cin, taps, None), "oihw_to_tap_major_t")
    check(lib.glf_tap_major_to_oihw(tm.ptr, back.ptr, cout, cin, taps, None), "tap_major_to_oihw")
    sync()
    guards(tm, tmt, back, what=f"re-layout {cout} x {cin} x {taps}")
    r1, r2 = R.relayout_refs(w)
    exact(tm.dense(), dev(row(r1)), False, "oihw_to_tap_major", "re-layout")
    exact(tmt.dense(), dev(row(r2)), False, "oihw_to_tap_major_t", "re-layout")
    exact(back.dense(), dev(row(w)), False, "tap_major_to_oihw(oihw_to_tap_major(w))", "re-layout")
    refused(lib, lib.glf_oihw_to_tap_major(ptr(wb), tm.ptr, cout, 0, taps, None), ERR_BAD_SHAPE, "oihw_to_tap_major: bad shape")


def test_weight_relayout_second_trip(L, BIG):
    lib, check = L
    cout, cin, taps = 64, (BIG + 64 * 9 - 1) // (64 * 9), 9
    n = cout * cin * taps
    w = R.gauss32((cout, cin, taps), 572)
    wb = put32(row(w))
    tm, tmt, back = Guarded(1, n), Guarded(1, n), Guarded(1, n)
    check(lib.glf_oihw_to_tap_major(ptr(wb), tm.ptr, cout, cin, taps, None), "oihw_to_tap_major")
    check(lib.glf_oihw_to_tap_major_t(ptr(wb), tmt.ptr, cout, cin, taps, None), "oihw_to_tap_major_t")
    check(lib.glf_tap_major_to_oihw(tm.ptr, back.ptr, cout, cin, taps, None), "tap_major_to_oihw")
    sync()
    guards(tm, tmt, back, what="re-layout big")
    r1, r2 = R.relayout_refs(w)
    exact(tm.dense(), dev(row(r1)), False, "oihw_to_tap_major big", "re-layout")
    exact(tmt.dense(), dev(row(r2)), False, "oihw_to_tap_major_t big", "re-layout")
    exact(back.dense(), dev(row(w)), False, "round trip big", "re-layout")


# ------------------------------------------------------------------------------------------- amax_combine, counter_add
def test_amax_combine_and_counter_add(L):
    lib, check = L
    cases = [  # a, b, scale, sum, start, want
        (-3.0, 2.0, 1.0, 0, 0.0, 3.0), (-3.0, 2.0, 1.0, 1, 0.0, 5.0), (-3.0, None, 2.0, 0, 0.0, 6.0), (-3.0, None, 2.0, 1, 1.0, 6.0),
        (-3.0, -4.0, 0.5, 1, 0.0, 3.5), (3.0, 4.0, 0.0, 1, 0.0, 0.0), (3.0, 4.0, 0.0, 0, 2.0, 2.0), (3.0, 4.0, 1.0, 1, 8.0, 8.0), (3.0, 4.0, 1.0, 0, 8.0, 8.0),
    ]
    for a, b, scale, s, start, want in cases:
        out = Guarded(1, 1).fill(torch.tensor([[start]]))
        at = torch.tensor([a], dtype=F32, device=DEV)
        bt = None if b is None else torch.tensor([b], dtype=F32, device=DEV)
        check(lib.glf_amax_combine(ptr(at), ptr(bt), scale, s, out.ptr, None), "amax_combine")
        sync()
        guards(out, what="amax_combine")
        assert float(out.t) == want, (a, b, scale, s, start, float(out.t), want)
    out = Guarded(1, 1)
    at = torch.ones(1, dtype=F32, device=DEV)
    refused(lib, lib.glf_amax_combine(ptr(at), None, -1.0, 0, out.ptr, None), ERR_BAD_SHAPE, "amax_combine: scale must be >= 0", out)
    refused(lib, lib.glf_amax_combine(None, None, 1.0, 0, out.ptr, None), ERR_NULL, "amax_combine: null argument", out)
    for start, inc, want in ((0, 5, 5), (7, 0, 7), (-1, 2, 1), (2 ** 62, 2 ** 62, -2 ** 63)):      # int64 views of uint64: -1 is 2^64 - 1
        ctr = Guarded(1, 1, dtype=torch.int64).fill(torch.tensor([[start]], dtype=torch.int64))
        check(lib.glf_counter_add(ctr.ptr, inc, None), "counter_add")
        sync()
        assert ctr.intact() and ctr.written() and int(ctr.t) == want, (start, inc, int(ctr.t))
    refused(lib, lib.glf_counter_add(None, 1, None), ERR_NULL, "counter_add: null argument")
