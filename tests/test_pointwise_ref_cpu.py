"""CPU side of the pointwise gate (tests/pointwise_ref.py, tests/test_gpu_pointwise.py): every reference against torch in float64 at
the shapes the GPU tests use, the exactness / bf16-representability preconditions of the integer families, the gate's tie
condition and overlap's threshold condition on the generated inputs, the restated dropout hash (against its scalar definition
and statistically), torch's own fp32 evaluation of each transcendental formula inside the stated intervals, and the gates' teeth."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pointwise_ref as R
from pointwise_ref import BF, F32, F64, U


def inside(got, ref, mag, k, bf16=False, extra=0.0):
    d = (k + 4) * U * mag + extra
    if bf16:
        return bool(((got >= R.bf16_rne(ref - d)) & (got <= R.bf16_rne(ref + d))).all())
    return bool(((got.double() - ref).abs() <= d).all())


def inside_rel(got, ref, kelem, extra=0.0):
    return bool(((got.double() - ref).abs() <= (kelem + 4) * U * ref.abs() + extra).all())


# ----------------------------------------------------------------------------------------------------------------- dropout
def test_hash_restatement_matches_its_scalar_definition_and_wraps():
    for seed in R.DROP_SEED + [2 ** 64 - 1]:
        for step in R.DROP_STEP + [2 ** 64 - 1]:
            h = R.dropout_hash(seed, step, 300)
            base = (R.effective_seed(seed, step) * 0x100000001B3) & (2 ** 64 - 1)
            for i in (0, 1, 7, 8, 255, 299):
                assert int(h[i]) == R.mix64_scalar((base + i) & (2 ** 64 - 1)), (seed, step, i)
            assert int(h.max()) < 2 ** 24
    assert R.effective_seed(5, None) == R.effective_seed(5, 0) == 5
    assert int(R.dropout_threshold(0.0)) == 0 and int(R.dropout_threshold(0.5)) == 2 ** 23 and int(R.dropout_threshold(0.999)) == int(np.float32(0.999) * np.float32(2 ** 24))


def test_hash_kept_share_is_binomial():
    n = 2 ** 20
    for seed in R.DROP_SEED:
        for step in (None, 3):
            for p in R.DROP_P:
                share = float(R.dropout_keep(seed, step, n, p).double().mean())
                q = 1.0 - int(R.dropout_threshold(p)) / 2.0 ** 24
                assert abs(share - q) <= 4.0 * math.sqrt(max(q * (1 - q), 0.0) / n) + 1e-12, (seed, step, p, share)
                assert abs(q - (1 - p)) <= 2.0 ** -23


def test_dropout_reference_and_teeth():
    for st in ("f32", "bf16"):
        x = R.dropout_input(st, 264)
        assert bool((x != 0).all())
        keep = R.dropout_keep(1, 3, 264, 0.5)
        y = R.dropout_ref(x, keep, 0.5)
        assert torch.equal(y, torch.where(keep, 2.0 * x, torch.zeros_like(x)))
        y9 = R.dropout_ref(x, keep, 0.9)
        assert torch.equal(y9.float().double(), y9) and torch.equal(y9[~keep], torch.zeros(int((~keep).sum()), dtype=F64))
    # a mask hashed per access (index i * W) is not the mask; another step is another mask
    assert not torch.equal(R.dropout_keep(1, 3, 264, 0.5), R.dropout_keep(1, 3, 264, 0.5, per_access=8))
    assert not torch.equal(R.dropout_keep(1, 3, 264, 0.5), R.dropout_keep(1, 4, 264, 0.5))
    assert not torch.equal(R.dropout_keep(1, 3, 264, 0.5), R.dropout_keep(2, 3, 264, 0.5))


# ------------------------------------------------------------------------------------------ relu, axpby, add_n, frames
def test_elementwise_references_and_preconditions():
    for st in ("f32", "bf16"):
        for numel in R.RELU_NUMEL:
            x, dy = R.relu_inputs(st, numel)
            assert torch.equal(R.relu_fwd_ref(x), torch.relu(x)) and not bool(x.isnan().any())
            xr = x.clone().requires_grad_(True)
            torch.relu(xr).backward(dy)
            assert torch.equal(R.relu_bwd_ref(dy, x), xr.grad)
            if st == "bf16":
                assert torch.equal(x.to(BF).double(), x)
        sp = R.relu_specials(st)
        assert bool((sp == float("inf")).any()) and bool(((sp != 0) & (sp.abs() < R.TINY)).any()) and bool((sp == 0).sum() == 2)
    x, y = R.ints((1027,), 111, -3, 3), R.ints((1027,), 112, -3, 3)
    for a, b in R.AXPBY_COEF:
        ref, mag = R.axpby_ref(x, y, a, b)
        R.assert_exact(mag)
        assert torch.equal(R.bf16_rne(ref), ref) and float(ref.abs().max()) <= 256
        assert torch.equal(ref, torch.add(a * x, y, alpha=b))
    g, h = R.gauss32((1027,), 113, 2.0, 0.3), R.gauss32((1027,), 114, 1.0, -0.2)
    a, b = float(np.float32(0.75)), float(np.float32(-1.3))
    ref, mag = R.axpby_ref(g, h, a, b)
    got = torch.tensor(a, dtype=F32) * g.float() + torch.tensor(b, dtype=F32) * h.float()
    assert inside(got, ref, mag, R.K_AXPBY)
    assert not inside(torch.roll(got, 1), ref, mag, R.K_AXPBY), "a result shifted by one element must be rejected"
    xs = [R.ints((1032,), 120 + j, -3, 3) for j in range(8)]
    ref, mag = R.add_n_ref(xs)
    R.assert_exact(mag)
    assert torch.equal(R.bf16_rne(ref), ref) and torch.equal(ref, torch.stack(xs).sum(0))


# ---------------------------------------------------------------------------------------------------------------- max-pool
def _pool_brute(x, ge=False):
    """window code by scanning the nine taps in order: first in-range element, then strictly greater or NaN replaces (ge: the
    defect 'greater or equal')"""
    n, h, w, c = x.shape
    ho, wo = R.pool_out(h), R.pool_out(w)
    y = torch.empty(n, ho, wo, c, dtype=F64)
    code = torch.empty(n, ho, wo, c, dtype=torch.uint8)
    for oy in range(ho):
        for ox in range(wo):
            best, bi, first = None, None, True
            for ky in range(3):
                for kx in range(3):
                    iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                    if iy < 0 or iy >= h or ix < 0 or ix >= w:
                        continue
                    v = x[:, iy, ix, :]
                    if first:
                        best, bi, first = v.clone(), torch.full(v.shape, ky * 3 + kx, dtype=torch.uint8), False
                    else:
                        take = ((v >= best) if ge else (v > best)) | v.isnan()
                        best, bi = torch.where(take, v, best), torch.where(take, torch.tensor(ky * 3 + kx, dtype=torch.uint8), bi)
            y[:, oy, ox, :], code[:, oy, ox, :] = best, bi
    return y, code


@pytest.mark.parametrize("kind", ["plain", "relu", "special"])
def test_maxpool_reference(kind):
    for n, h, w in R.POOL_SHAPES:
        for c in (4, 8, 12):
            x = R.pool_input(n, h, w, c, kind)
            assert torch.equal(x.to(BF).double()[~x.isnan()], x[~x.isnan()])
            y, code, ind = R.maxpool_ref(x)
            yb, cb = _pool_brute(x)
            assert R.same_values(y, yb) and torch.equal(code, cb), (kind, n, h, w, c)
            dy = R.ints(tuple(y.shape), 302, -2, 2)
            dx = R.maxpool_bwd_ref(dy, ind, h, w)
            assert float(dx.abs().max()) <= 8 and torch.equal(R.bf16_rne(dx), dx)
            assert float(dx.sum()) == float(dy.sum())
            if kind != "special":
                xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
                F.max_pool2d(xr, 3, 2, 1).backward(dy.permute(0, 3, 1, 2))
                assert torch.equal(dx, xr.grad.permute(0, 2, 3, 1))
            if kind == "special" and h >= 4 and w >= 4:
                assert bool(x.isnan().any()) and bool((x == float("-inf")).any())
                assert int(code[0, 1, 1, 0]) == 0 and int(code[0, 1, 1, 1]) == 8      # NaN in the first tap, in the last tap
    # teeth: `>=` (the last maximum wins) gives other codes wherever there are ties
    for n, h, w in R.POOL_SHAPES[1:]:
        x = R.pool_input(n, h, w, 8, "plain")
        y, code, _ = R.maxpool_ref(x)
        y2, code2 = _pool_brute(x, ge=True)
        assert torch.equal(y, y2) and not torch.equal(code, code2), (n, h, w)


# ------------------------------------------------------------------------------------------------- row sums and broadcasts
def test_rows_references_preconditions_and_kernel_choice():
    for n in R.ROWS_N:
        for p in R.ROWS_P:
            for c in (1, 4, 260):
                x = R.ints((n * p, c), 521, -3, 3)
                ref, mag = R.sum_rows_ref(x, n, p, 0.5)
                R.assert_exact(2 * mag)
                assert torch.equal(ref, 0.5 * torch.stack([x[i * p:(i + 1) * p].sum(0) for i in range(n)]))
                g = R.gauss32((n * p, c), 522, 2.0, 0.7)
                ref, mag = R.sum_rows_ref(g, n, p, 0.5)
                seq = 0.5 * g.float().view(n, p, c).sum(1)            # some fp32 order
                assert inside(seq, ref, mag, R.k_sum_rows(p, False))
                xb = R.ints((n, c), 531, -3, 3)
                y0 = R.ints((n * p, c), 533, -2, 2)
                ref, mag = R.bcast_ref(xb, p, 0.5, y0)
                R.assert_exact(mag)
                assert torch.equal(ref, y0 + 0.5 * xb[torch.arange(n * p) // p])
                ref, _ = R.bcast_ref(xb, p, 0.5)
                assert torch.equal(R.bf16_rne(ref), ref)
    assert R.k_sum_rows(196, False) == 49 + 4 and R.k_sum_rows(196, True) == 1
    assert R.sum_rows_uses_double(64, 64) and R.sum_rows_uses_double(260, 264) and not R.sum_rows_uses_double(64, 65)
    assert not R.sum_rows_uses_double(3, 4) and not R.sum_rows_uses_double(64, 64, base_off=1)
    # teeth: three of the four row lanes
    g = R.gauss32((196, 3), 523, 2.0, 0.7)
    ref, mag = R.sum_rows_ref(g, 1, 196, 0.5)
    lanes3 = 0.5 * g[torch.arange(196) % 4 != 3].sum(0, keepdim=True)
    assert not inside(lanes3, ref, mag, R.k_sum_rows(196, False))


# ----------------------------------------------------------------------------------------------------------------- softmax
def test_softmax_reference_and_fp32_evaluation():
    for rows in R.SOFT_ROWS:
        for cols in R.SOFT_COLS:
            x = R.softmax_input(rows, cols)
            assert torch.equal(x.float().double(), x)
            if cols > 1:
                j = int(x[0].argmax())
                rest = torch.cat([x[0, :j], x[0, j + 1:]])
                assert float(x[0, j] - rest.max()) >= 60 - 1e-5
            p, kel = R.softmax_ref(x)
            assert torch.allclose(p, torch.softmax(x, 1), rtol=1e-13, atol=0)
            x32 = x.float()
            e32 = torch.exp(x32 - x32.max(1, keepdim=True).values)
            got = e32 * (1.0 / e32.sum(1, keepdim=True))
            assert inside_rel(got, p, kel, R.TINY), (rows, cols)
            assert inside_rel(torch.softmax(x32, 1), p, kel, R.TINY), (rows, cols)
            if cols > 2:
                assert not inside_rel(torch.roll(got, 1, 1), p, kel, R.TINY)
            for fam in ("int", "gauss"):
                pp, dy = R.softmax_bwd_inputs(fam, rows, cols)
                ref, mag = R.softmax_bwd_ref(pp, dy)
                if fam == "gauss":
                    lg = R.gauss32((rows, cols), 411, 2.0).requires_grad_(True)
                    sm = torch.softmax(lg, 1)
                    sm.backward(dy)
                    p64 = sm.detach()
                    r64, _ = R.softmax_bwd_ref(p64, dy)
                    assert torch.allclose(r64, lg.grad, rtol=1e-10, atol=1e-14)
                    got = pp.float() * (dy.float() - (pp.float() * dy.float()).sum(1, keepdim=True))
                    assert inside(got, ref, mag, R.k_softmax_bwd(cols))
                else:
                    R.assert_exact(mag)
                    assert torch.equal(ref.float().double(), ref)


# ---------------------------------------------------------------------------------------------------------------- bilinear
@pytest.mark.parametrize("shape", R.BIL_SHAPES + [(5, 7, 725, 725), (363, 363, 400, 380)])
def test_bilinear_restatement_against_interpolate(shape):
    h, w, ho, wo = shape
    for osz, isz in ((ho, h), (wo, w)):
        a0, a1, al = R.bil_index(osz, isz)
        b0, b1, bl = R.bil_index(osz, isz, fused=True)
        assert torch.equal(a0, b0) and torch.equal(a1, b1), "the fused coordinate picks other source pixels"
        assert bool(((al - bl).abs() <= max(1, isz) * U).all())
        assert bool((al >= 0).all()) and bool((al <= 1).all() or isz == 1)
    n, c = (2, 5) if h * w < 1000 else (1, 1)
    x = R.gauss32((n, h, w, c), 552, 2.0, 0.5)
    ref, mag = R.bilinear_fwd_ref(x, ho, wo)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.interpolate(xr, size=(ho, wo), mode="bilinear", align_corners=False)
    if h > 1 and w > 1:                       # with one source row ATen's lambda is irrelevant; ours keeps (1 - l) + l
        assert bool(((y.detach() - ref).abs() <= 16 * (h + w) * U * mag + 1e-300).all())
    dy = R.gauss32((n, c, ho, wo), 554, 1.0, 0.2)
    y.backward(dy)
    dref, dmag, rc, cc = R.bilinear_bwd_ref(dy, h, w)
    assert bool(((xr.grad.permute(0, 2, 3, 1) - dref).abs() <= 16 * (h + w) * U * dmag + 1e-300).all())
    assert torch.allclose((ref * dy).sum(), (dref * x).sum(), rtol=1e-12), "backward is not the adjoint of forward"
    assert rc <= int(2.0 * ho / h) + 4 + 1 and cc <= int(2.0 * wo / w) + 4 + 1, "more contributing outputs than the kernel's window holds"
    y32 = F.interpolate(x.permute(0, 3, 1, 2).float(), size=(ho, wo), mode="bilinear", align_corners=False)
    assert inside(y32, ref, mag, R.k_bilinear_fwd(h, w))
    if (h, w) == (ho, wo):
        assert torch.equal(ref, x.permute(0, 3, 1, 2)) and torch.equal(dref, dy.permute(0, 2, 3, 1))
    elif h * w > 1 and ho * wo > 4:
        assert not inside(torch.roll(y32, 1, 3), ref, mag, R.k_bilinear_fwd(h, w)) or wo == 1


# --------------------------------------------------------------------------------------------------------------------- gate
def test_gate_reference_conditions_and_fp32_evaluation():
    w = R.GATE_WEIGHT
    for rows in R.GATE_ROWS:
        for ncls in R.GATE_NCLS:
            cls, ctr = R.gate_inputs(rows, ncls)
            assert float(cls.abs().max()) <= 8 and R.gate_conditions(cls)
            if ncls > 1:
                top = cls.max(1, keepdim=True).values
                assert bool(((cls == top).sum(1)[::3] >= 2).all()), "no bit-equal maxima planted"
            bi, a, ka = R.gate_fwd_ref(cls, ctr, w)
            clsr, ctrr = cls.clone().requires_grad_(True), ctr.clone().requires_grad_(True)
            best = torch.sigmoid(clsr).max(1).values
            a_t = torch.sigmoid(w * best * torch.sigmoid(ctrr))
            assert torch.allclose(a, a_t.detach(), rtol=1e-14)
            assert bool((cls.gather(1, bi.long().view(-1, 1))[:, 0] == cls.max(1).values).all())
            first = torch.stack([(cls[r] == cls[r].max()).nonzero()[0, 0] for r in range(rows)])
            assert torch.equal(bi.long(), first)
            # torch's fp32 evaluation of the same formula
            s32 = 1.0 / (1.0 + torch.exp(-cls.float()))
            a32 = 1.0 / (1.0 + torch.exp(-(torch.tensor(w, dtype=F32) * s32.max(1).values * (1.0 / (1.0 + torch.exp(-ctr.float()))))))
            assert inside_rel(a32, a, ka)
            assert torch.equal(torch.stack([(s32[r] == s32[r].max()).nonzero()[0, 0] for r in range(rows)]), first)
            if rows > 1:
                d = (ka + 4) * U * a
                assert bool(((a[1:] - a[:-1]).abs() > 2 * torch.maximum(d[1:], d[:-1])).float().mean() > 0.9), "rows do not differ strongly"
                assert not inside_rel(torch.roll(a32, 1), a, ka), "a neighbour's a must be rejected"
            c = 264
            for st in ("f32", "bf16"):
                for fam in ("int", "gauss"):
                    f = R.ints((rows, c), 511, -3, 3) if fam == "int" else R.gaussian(st, (rows, c), 511, 2.0, 0.3)
                    dy = R.ints((rows, c), 512, -2, 2) if fam == "int" else R.gaussian(st, (rows, c), 512, 1.0, 0.1)
                    a_in = a.float().double()
                    b = R.gate_bwd_ref(dy, f, cls, ctr, a_in, bi, w)
                    if st == "f32" and fam == "gauss":
                        fr = f.clone().requires_grad_(True)
                        (fr * a_t[:, None]).backward(dy)
                        # autograd routes a tie's gradient as torch.max does; compare on the argmax column torch took
                        tb = torch.sigmoid(cls).max(1).indices
                        same = tb == bi.long()
                        g = clsr.grad.gather(1, bi.long().view(-1, 1))[:, 0]
                        assert torch.allclose(g[same], b.dcls.sum(1)[same], rtol=1e-6, atol=1e-12)
                        assert torch.allclose(ctrr.grad, b.dctr, rtol=1e-6, atol=1e-12)
                        assert torch.allclose(fr.grad, dy * a_t.detach()[:, None], rtol=1e-12)
                        clsr.grad = None
                        ctrr.grad = None
                        a_t = torch.sigmoid(w * torch.sigmoid(clsr).max(1).values * torch.sigmoid(ctrr))
                        # fp32 evaluation of the kernel's expression
                        da = (dy.float() * f.float()).sum(1)
                        m32 = s32.gather(1, bi.long().view(-1, 1))[:, 0]
                        c32 = 1.0 / (1.0 + torch.exp(-ctr.float()))
                        af = a_in.float()
                        dt = da * af * (1 - af) * w
                        kda = R.k_gate_da(st, c, fam) + c           # torch's row sum: some order, at most c adds
                        assert inside((dt * c32 * m32 * (1 - m32)).double(), b.dcls.sum(1), b.dclsm.sum(1) * (kda + b.kcls + 4) / 4, 0)
                        assert inside((dt * m32 * c32 * (1 - c32)).double(), b.dctr, b.dctrm * (kda + b.kctr + 4) / 4, 0)
                    if fam == "int":
                        R.assert_exact((dy * f).abs().sum(1))
                    y = R.product32(f, a_in[:, None])
                    assert torch.equal(y, (f.float() * a_in.float()[:, None]).double())


# ------------------------------------------------------------------------------------------------------------ BCE, overlap
def test_bce_and_overlap_reference_conditions_and_fp32_evaluation():
    for numel in R.BCE_NUMEL + [R.big()]:
        x, t = R.bce_inputs(numel)
        assert R.overlap_condition(x) and torch.equal(x.float().double(), x)
        if numel >= 7:
            assert all(bool((x == v).any()) for v in R.BCE_PLANTS) and bool((t == 0.25).any()) == (numel > 1) or numel < 63
        g = 1.0 / 256
        loss, mag, dx, dmag = R.bce_ref(x, t, g)
        xr = x.clone().requires_grad_(True)
        lt = F.binary_cross_entropy_with_logits(xr, t, reduction="sum")
        (lt * g).backward()
        assert torch.allclose(loss, lt.detach(), rtol=1e-13) and torch.allclose(dx, xr.grad, rtol=1e-12, atol=1e-300)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dx).all())
        x32, t32 = x.float(), t.float()
        terms = torch.clamp_min(x32, 0) - x32 * t32 + torch.log1p(torch.exp(-x32.abs()))
        assert inside(terms.double().sum(), loss, mag, R.K_BCE)
        d32 = (1.0 / (1.0 + torch.exp(-x32)) - t32) * torch.tensor(g, dtype=F32)
        assert inside(d32, dx, dmag, R.K_BCE_DX, extra=R.TINY * g) and bool(torch.isfinite(d32).all())
        want = R.overlap_ref(x, t)
        pr = (1.0 / (1.0 + torch.exp(-x32))) > 0.5
        got = torch.tensor([int((pr & (t != 0)).sum()), int((pr & (t == 0)).sum()), int((~pr & (t != 0)).sum()), int((~pr & (t == 0)).sum())])
        assert torch.equal(got, want) and int(want.sum()) == numel
        if numel >= 63:
            assert not inside(torch.roll(d32, 1), dx, dmag, R.K_BCE_DX, extra=R.TINY * g)


# -------------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("shape", R.STEM_SHAPES)
def test_stem_references_and_preconditions(shape):
    h, w, pad = shape
    for n in R.STEM_N:
        for fam in ("int", "gauss"):
            I = R.stem_inputs(fam, n, h, w, pad)
            y, ymag = R.stem_fwd_ref(I.x, I.w, I.bias, pad)
            assert tuple(y.shape) == (n, I.ho, I.wo, 64)
            # direct definition at a few pixels
            xp = F.pad(I.x, (pad, pad, pad, pad))
            for (oy, ox) in {(0, 0), (I.ho - 1, I.wo - 1), (I.ho // 2, I.wo // 3)}:
                patch = xp[:, oy:oy + 7, ox:ox + 7].reshape(n, 49)
                assert torch.allclose(y[:, oy, ox, :], patch @ I.w.t() + I.bias, rtol=1e-12, atol=1e-12)
            dw, dwm, db, dbm = R.stem_wgrad_ref(I.x, I.dy, pad)
            wr, br = I.w.clone().requires_grad_(True), I.bias.clone().requires_grad_(True)
            F.conv2d(I.x[:, None], wr.view(64, 1, 7, 7), br, padding=pad).backward(I.dy.permute(0, 3, 1, 2))
            assert torch.allclose(dw, wr.grad, rtol=1e-12, atol=1e-12) and torch.allclose(db, br.grad, rtol=1e-12, atol=1e-12)
            pool, pmag = R.stem_pool_ref(y, ymag, I.mean, I.invstd, I.gamma, I.beta)
            bn = F.batch_norm(y.permute(0, 3, 1, 2), I.mean, 1.0 / I.invstd ** 2, I.gamma, I.beta, False, 0.0, 1e-300)
            assert torch.allclose(pool.permute(0, 3, 1, 2), F.max_pool2d(torch.relu(bn), 3, 2, 1), rtol=1e-12, atol=1e-12)
            assert tuple(pool.shape) == (n, (I.ho - 1) // 2 + 1, (I.wo - 1) // 2 + 1, 64)
            if fam == "int":
                R.assert_exact(ymag, dwm, dbm, pmag)
                assert float(y.abs().max()) <= 50 and torch.equal(R.bf16_rne(y), y) and torch.equal(I.dy.to(BF).double(), I.dy)
                assert torch.equal(pool.float().double(), pool)
            else:
                y32 = F.conv2d(I.x.float()[:, None], I.w.float().view(64, 1, 7, 7), I.bias.float(), padding=pad).permute(0, 2, 3, 1)
                assert inside(y32, y, ymag, R.K_STEM_FWD)
                assert inside(y32.to(BF).double(), y, ymag, R.K_STEM_FWD, bf16=True)
                if I.wo > 1:
                    assert not inside(torch.roll(y32, 1, 2), y, ymag, R.K_STEM_FWD)
    assert R.k_stem_wgrad(17, 32) == 257 and R.k_stem_wgrad(1, 1) == 2


# --------------------------------------------------------------------------------------------- transposes and re-layouts
def test_layout_references():
    for cout, cin, taps in R.RELAYOUT:
        w = R.gauss32((cout, cin, taps), 571)
        r1, r2 = R.relayout_refs(w)
        assert torch.equal(r1.permute(1, 2, 0), w) and torch.equal(r2.permute(2, 1, 0), w)
        assert float(r1[taps - 1, cout - 1, 0]) == float(w[cout - 1, 0, taps - 1]) and float(r2[taps - 1, 0, cout - 1]) == float(w[cout - 1, 0, taps - 1])
    for st in ("f32", "bf16"):
        for rows in R.TR_DIMS[st]:
            pads = R.rows_pads(rows, R.TR_TILE[st])
            assert pads[0] == rows and rows + 1 in pads and pads[-1] % R.TR_TILE[st] == 1
    live, off = R.strided_live(3, 5, 4, 7, 40)
    assert live.numel() == 2 * 40 + 4 * 7 + 4 and int(live.sum()) == 60 and int(off[4]) == 7 and int(off[20]) == 40
    assert R.big() == 8 * 256 * 256 + 773 and R.big(304) == 8 * 304 * 256 + 773
