"""CPU: the references, preconditions and gates of tests/test_gpu_s16_stream.py (helpers in tests/s16_stream_ref.py).

The float64 references reproduce torch in float64 (forward and autograd) to 1e-12; the integer family is exact in fp32 and has no
unsure ReLU sign at every shape the GPU tests run; the gauss family stays under the unsure-sign cap at every such shape; the
interval gate rejects a value one bf16 ulp outside and accepts one on the edge; the guarded buffers notice a stray store."""
import pytest
import torch
import torch.nn.functional as F

import s16_stream_ref as R

F64 = torch.float64


def _same(a, b, what):
    err = float((a - b).abs().max())
    assert err <= 1e-12 * max(1.0, float(b.abs().max())), (what, err)


@pytest.mark.parametrize("family", ["int", "gauss"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("has_res", [False, True])
def test_batchnorm_references_reproduce_torch(family, training, has_res):
    rows, c = 70, 24
    i = R.bn_inputs(family, rows, c, "cpu")
    x, res = i.x.clone().requires_grad_(True), i.res.clone().requires_grad_(True)
    gamma, beta = i.gamma.clone().requires_grad_(True), i.beta.clone().requires_grad_(True)
    sums, _ = R.colstats_ref(i.x)
    if training:
        mean, invstd, unb = R.bn_stats_from_sums(sums, rows)
        rm, rv = torch.zeros(c, dtype=F64), torch.ones(c, dtype=F64)
        y = F.batch_norm(x, rm, rv, gamma, beta, True, R.MOM, R.EPS)
        _same(rm, R.MOM * mean, "running_mean")
        _same(rv, (1 - R.MOM) + R.MOM * unb, "running_var")
    else:
        mean, invstd = i.mean, i.invstd
        y = F.batch_norm(x, mean.clone(), 1.0 / invstd ** 2 - R.EPS, gamma, beta, False, R.MOM, R.EPS)
    y = torch.relu(y + res if has_res else y)
    up = i.dy + i.dy2
    grads = torch.autograd.grad(y, [x, gamma, beta] + ([res] if has_res else []), up)
    v, _ = R.bn_fwd_ref(i.x, mean, invstd, i.gamma, i.beta, i.res if has_res else None)
    _same(torch.relu(v), y.detach(), "y")
    b = R.bn_bwd_ref(i.dy, i.dy2, i.x, mean, invstd, (v > 0).double())
    dx = R.bn_bwd_dx_train(b, i.gamma, invstd, b.s1, b.s2, rows)[0] if training else R.bn_bwd_dx_eval(b, i.gamma, invstd)[0]
    _same(dx, grads[0], "dx")
    _same(b.s2, grads[1], "dgamma")
    _same(b.s1, grads[2], "dbeta")
    if has_res:
        _same(b.g, grads[3], "dres")


@pytest.mark.parametrize("family", ["int", "gauss"])
def test_tail_references_reproduce_torch(family):
    rows, c = 17, 520
    i = R.tail_inputs(family, rows, c, "cpu")
    w, x = i.w.clone().requires_grad_(True), i.x.clone().requires_grad_(True)
    ln_g, ln_b = i.ln_g.clone().requires_grad_(True), i.ln_b.clone().requires_grad_(True)
    u_t = F.batch_norm(w, i.mean.clone(), 1.0 / i.invstd ** 2 - R.EPS, i.bn_g, i.bn_b, False, R.MOM, R.EPS) + x
    z = F.layer_norm(u_t, (c,), ln_g, ln_b, R.LN_EPS)
    du_t, dg_t, db_t = torch.autograd.grad(z, [x, ln_g, ln_b], i.dz)
    u, umag = R.tail_u(i)
    _same(u, u_t.detach(), "u")
    mean, _ = R.tail_row_mean(u, umag)
    rstd, _ = R.tail_row_rstd(u, umag, mean)
    _same(mean, u_t.detach().mean(1), "row_mean")
    _same(rstd, 1.0 / torch.sqrt(u_t.detach().var(1, unbiased=False) + R.LN_EPS), "row_rstd")
    _same(R.tail_z(u, umag, mean, rstd, i.ln_g, i.ln_b)[0], z.detach(), "z")
    b = R.tail_bwd_ref(u, umag, i.dz, mean, rstd, i.ln_g)
    _same(b.du, du_t, "du")
    _same(b.dg, dg_t, "dln_gamma")
    _same(b.db, db_t, "dln_beta")


def test_magnitudes_dominate_their_references():
    i = R.bn_inputs("gauss", 70, 24, "cpu")
    v, mag = R.bn_fwd_ref(i.x, i.mean, i.invstd, i.gamma, i.beta, i.res)
    assert bool((mag >= v.abs()).all())
    b = R.bn_bwd_ref(i.dy, i.dy2, i.x, i.mean, i.invstd, (v > 0).double())
    for r, m in ((b.g, b.gmag), (b.s1, b.s1mag), (b.s2, b.s2mag), R.bn_bwd_dx_eval(b, i.gamma, i.invstd), R.bn_bwd_dx_train(b, i.gamma, i.invstd, b.s1, b.s2, 70)):
        assert bool((m >= r.abs() * (1 - 1e-12)).all())
    t = R.tail_inputs("gauss", 17, 520, "cpu")
    u, umag = R.tail_u(t)
    mean, mmag = R.tail_row_mean(u, umag)
    rstd, rmag = R.tail_row_rstd(u, umag, mean)
    bw = R.tail_bwd_ref(u, umag, t.dz, mean, rstd, t.ln_g)
    for r, m in ((mean, mmag), (rstd, rmag), R.tail_z(u, umag, mean, rstd, t.ln_g, t.ln_b), (bw.du, bw.dumag), (bw.dg, bw.dgmag), (bw.db, bw.dbmag)):
        assert bool((m >= r.abs() * (1 - 1e-12)).all())


def test_reduction_geometry_covers_the_thread_mappings():
    assert [R.red_geometry(297, c)[0] for c in R.CHANNELS] == [1, 3, 9, 16, 16, 16, 16]
    assert R.red_geometry(297, 24)[1] == 85                                       # 85 row lanes, one idle thread
    assert R.red_geometry(*R.BIG_SHAPE)[2] == 32 and R.red_geometry(8500, 4096)[4] == 17     # the slice cap: 1 024 / 32 column blocks
    assert R.red_geometry(4100, 2048)[2] == 17 and R.red_geometry(1, 8)[2:] == (1, 1, 1)
    assert {R.red_geometry(r, 128)[2] for r in R.ROWS} == {1, 2, 5, 17}          # several slices with a ragged last one
    # fp32 storage, four elements per access: 64 column blocks cap 4 100 rows at 16 slices of 257 rows -- 17 rows per thread, four
    # unrolled trips and a one-row tail
    assert R.red_geometry(4100, 4096, 4) == (16, 16, 16, 257, 17)
    assert [R.red_geometry(297, c, 4)[0] for c in (4, 8, 72, 136)] == [1, 2, 16, 16]
    assert all(r * c <= 1031 * 4096 or (r, c) == (4100, 2048) for r, c in R.BN_SHAPES) and len(R.BN_SHAPES) == 41


@pytest.mark.parametrize("rows,c", R.BN_SHAPES)
def test_integer_family_is_exact_and_sure_at_every_batchnorm_shape(rows, c):
    i = R.bn_inputs("int", rows, c, "cpu")
    _, smag = R.colstats_ref(i.x)
    R.assert_exact(smag)
    for res in (None, i.res):
        v, mag = R.bn_fwd_ref(i.x, i.mean, i.invstd, i.gamma, i.beta, res)
        assert not bool(R.unsure_of(v, mag, R.K_Y).any()) and float(v.abs().min()) >= 0.125
    b = R.bn_bwd_ref(i.dy, i.dy2, i.x, i.mean, i.invstd, None)
    # every term is a multiple of 1/2 (g (x - mean) invstd) or 1/4 (g gamma invstd): exact while the magnitude stays below 2^24 / 4
    R.assert_exact(b.s1mag, 4 * b.s2mag, 4 * R.bn_bwd_dx_eval(b, i.gamma, i.invstd)[1])
    assert torch.equal(b.s2 * 2, (b.s2 * 2).round()) and torch.equal(b.s1, b.s1.round())


def test_integer_family_is_exact_at_the_slice_cap_shape():
    """from the value ranges alone (the GPU test asserts it on the data): |g| <= 4, |x - mean| <= 4, invstd <= 2"""
    rows, _ = R.BIG_SHAPE
    R.assert_exact(torch.tensor([rows * 9.0, rows * 4.0, 4 * rows * 4.0 * 4.0 * 2.0]))
    assert rows * 9.0 < 3.5e4 * 2.3                                               # the x^2 sums reach about 3.4e4 (4 on average per row)


@pytest.mark.parametrize("rows,c", R.BN_SHAPES)
def test_gauss_family_meets_the_unsure_cap_at_every_batchnorm_shape(rows, c):
    i = R.bn_inputs("gauss", rows, c, "cpu")
    sums, _ = R.colstats_ref(i.x)
    mean_t, invstd_t, _ = R.bn_stats_from_sums(sums, rows)
    for mean, invstd in ((i.mean, i.invstd), (mean_t.float().double(), invstd_t.float().double())):
        for res in (None, i.res):
            v, mag = R.bn_fwd_ref(i.x, mean, invstd, i.gamma, i.beta, res)
            share = R.unsure_share(R.unsure_of(v, mag, R.K_Y))
            assert share <= R.UNSURE_CAP, (rows, c, share)


@pytest.mark.parametrize("c", R.TAIL_C)
def test_tail_and_row_sum_integer_preconditions(c):
    for rows in R.TAIL_ROWS:
        i = R.tail_inputs("int", rows, c, "cpu")
        R.assert_exact(i.dz.abs().sum(0))
    for n in R.SUM_N:
        for p in R.SUM_P:
            for cc in R.SUM_C:
                R.assert_exact(R.sum_rows_ref(R.sum_inputs("int", n, p, cc, "cpu"), n, p, 0.5)[1] * 2)


def test_interval_gate_edges():
    one = torch.tensor([1.0], dtype=F64)
    k = 5
    # bf16: around 1.0 the interval [1 - d, 1 + d] rounds to {1.0}; one bf16 ulp to either side is outside
    R.gate(torch.tensor([1.0]).to(R.BF), one, one, k, True, "on the edge", "t")
    for outside in (1.0 + 2.0 ** -7, 1.0 - 2.0 ** -8):
        with pytest.raises(AssertionError, match="outside the derived interval"):
            R.gate(torch.tensor([outside]).to(R.BF), one, one, k, True, "one ulp outside", "t")
    # a reference on a tie: both neighbours are inside, the next ones are not
    tie = one + 2.0 ** -8
    for inside in (1.0, 1.0 + 2.0 ** -7):
        R.gate(torch.tensor([inside]).to(R.BF), tie, one, k, True, "tie", "t")
    for outside in (1.0 - 2.0 ** -8, 1.0 + 2.0 ** -6):
        with pytest.raises(AssertionError):
            R.gate(torch.tensor([outside]).to(R.BF), tie, one, k, True, "tie", "t")
    # fp32: |got - ref| = d passes, one fp32 ulp more does not
    d = float(R.tol(k, one))
    assert d == 9 * 2.0 ** -23
    R.gate(torch.tensor([1.0 + d], dtype=F64), one, one, k, False, "edge", "t")
    with pytest.raises(AssertionError):
        R.gate(torch.tensor([1.0 + d + 2.0 ** -23], dtype=F64), one, one, k, False, "beyond", "t")
    # the `sure` selection and the absolute allowance
    R.gate(torch.tensor([1.0, 5.0], dtype=F64), torch.tensor([1.0, 1.0], dtype=F64), torch.ones(2, dtype=F64), k, False, "sure", "t",
           sure=torch.tensor([True, False]))
    R.gate(torch.tensor([1.5], dtype=F64), one, one, k, False, "extra", "t", extra=torch.tensor([0.5], dtype=F64))
    with pytest.raises(AssertionError):
        R.gate(torch.tensor([1.5 + 2 * d], dtype=F64), one, one, k, False, "extra", "t", extra=torch.tensor([0.5], dtype=F64))
    assert R.within_ulps(torch.tensor([1.0 + 2.0 ** -23]), one) and not R.within_ulps(torch.tensor([1.0 + 2.0 ** -22]), one)
    assert R.RATIOS.pop("t")[0] > 0


def test_exact_gate_rejects_one_wrong_element_and_a_truncating_store():
    ref = torch.tensor([257.0, 259.0, -3.5], dtype=F64)
    R.exact(torch.tensor([256.0, 260.0, -3.5]).to(R.BF), ref, True, "rne", "t")
    with pytest.raises(AssertionError):
        R.exact(torch.tensor([256.0, 258.0, -3.5]).to(R.BF), ref, True, "truncated", "t")
    with pytest.raises(AssertionError):
        R.exact(torch.tensor([257.0, 259.0, -3.0]), ref, False, "one wrong", "t")
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([2.0 ** 24]))
    R.RATIOS.pop("t (exact)")


def test_guarded_buffers_notice_stray_and_missing_stores():
    for make in (lambda: R.Guarded16(3, 8, 16, device="cpu"), lambda: R.Guarded(3, 8, 16, device="cpu"),
                 lambda: R.Guarded(3, 8, 16, dtype=torch.uint8, device="cpu"), lambda: R.Guarded(3, 8, 16, dtype=F64, device="cpu")):
        g = make()
        assert g.intact() and not g.written()
        g.fill(torch.ones(3, 8))
        assert g.intact() and g.written() and torch.equal(g.f64(), torch.ones(3, 8, dtype=F64))
        g.body[1, 8] = 0                                                          # the first pad column of row 1
        assert not g.intact()
        g = make()
        g.fill(torch.ones(3, 8))
        g.buf[R.GUARD - 1] = 0                                                    # the element in front
        assert not g.intact()
        g = make()
        g.fill(torch.ones(3, 8))
        g.t[2, 7] = g.sent                                                        # one element never stored
        assert not g.written()
    m = R.Guarded(1, 4, dtype=torch.uint8, device="cpu").fill(torch.tensor([[1, R.SENT_B, 3, 4]]))
    assert not m.written() and m.written(allow=torch.tensor([[False, True, False, False]]))
    assert R.Guarded16(2, 8, device="cpu").ptr % 16 == 0


def test_sign_bytes_and_cast_specials():
    pos = torch.zeros(2, 16, dtype=torch.bool)
    pos[0, 0] = pos[0, 9] = pos[1, 7] = True
    assert R.sign_bytes(pos).tolist() == [[1, 2], [128, 0]]
    s = R.cast_specials()
    assert s.numel() % 8 == 0 and not bool(s.view(torch.float32).isnan().any())
    f = s.view(torch.float32)
    b = f.to(R.BF)
    assert bool(b.isinf().sum() > f.isinf().sum())                                # a finite value that rounds to infinity is among them
    ties = (s & 0xFFFF) == 0x8000
    assert bool(ties.any()) and bool(((b.view(torch.int16)[ties] & 1) == 0).all())  # ties go to the even mantissa
    assert bool(R.cast_nans().view(torch.float32).isnan().all())


def test_pad_patterns_separate_every_pair_of_strided_operands():
    for pats, n in ((R.APPLY_PADS, 3), (R.BWD_PADS, 5)):
        assert len(pats) == n + 2 and all(len(v) == n and set(v) <= {0, 8} for v in pats.values())
        for i in range(n):
            assert {v[i] for v in pats.values()} == {0, 8}
            for j in range(i + 1, n):
                assert any(v[i] != v[j] for v in pats.values()), (i, j)
