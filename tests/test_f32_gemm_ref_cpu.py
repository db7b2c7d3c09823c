"""CPU: the reference, operand families, gates and case tables of tests/test_gpu_f32_gemm.py (tests/f32_gemm_ref.py) have teeth
before they judge a kernel.

  * the split emulation follows the definitions of csrc/split_f16.h and csrc/gemm_bf16s.hip (scale rule, ties to even, the
    models' residuals), and on the Gaussian cases |ideal - float64| stays inside the bounds the kernel headers claim;
  * the case tables reach every kernel variant (host formulas of the launchers); every integer run meets its exactness
    precondition and every Gaussian run the normal-pieces condition; the integer families make every kept product non-zero
    somewhere and every dropped one zero (but la * hb of the 13-bit f16 family, which is there to pin the split's rounding);
  * both gates accept the ideal result evaluated in fp32 in a shuffled order;
  * mutants built on the host.  The integer gate rejects every one of them; the Gaussian interval rejects every one it can by
    its derivation -- a result that is 2 ulp off lies inside ANY accumulation bound (2 < P n + 4) and is the integer gate's
    alone, and a truncating bf16 split is no mutant at all (three truncated 8-bit pieces hold all 24 bits of an fp32 value);
  * tightness: at one reduction row the interval rejects a bf16x6 result that lost any one of its three lowest products, which
    the elementwise 5e-5 gate of test_gpu_ops.py / test_gpu_rows_walk.py / test_gpu_tn_walk.py accepts."""
import pytest
import torch

import f32_gemm_ref as R

F32 = torch.float32
NT_SMALL = R.rows_case(33, 20, 32, bias=True, alpha=0.5)                           # one K tile, two 16-deep k-steps
NT_GATHER = R.rows_case(gather=1, conv=(1, 6, 5, 3, 1, 1, 1), N=12, K=32)          # 9 taps
TN_ONE = R.TN_CASES["k1_m64_n72"]                                                  # one reduction row
_DATA = {}


def data(c, arith, family):
    key = (id(c), arith, family)
    if key not in _DATA:
        _DATA[key] = R.make_data(c, arith, family)
    return _DATA[key]


def evaluate(c, d, arith, *, A=None, B=None, mask=None, **kw):
    """the result of the case as fp32, from possibly altered operands / tap mask / split / product list"""
    A, B, mask = d["A"] if A is None else A, d["B"] if B is None else B, d["mask"] if mask is None else mask
    P = torch.stack([R.ideal(c["mode"], A[b], B[b], d["src"], mask, arith, d["amax_a"], d["amax_b"], **kw)[0] for b in range(c["batch"])])
    return R.finish(P, P.abs(), d["alpha"], d["bias"], d["res"], d["relu"], d["cold"])[0].float()


def rejected(got, d):
    if d["exact"]:
        try:
            R.gate_exact(got, d["ref"], False, "mutant")
        except AssertionError:
            return True
        return False
    return bool(R.interval_violations(got, d["ref"], d["absref"], d["n_terms"], False)[0].any())


# ----------------------------------------------------------------------------------------
# the split emulation
# ----------------------------------------------------------------------------------------
def test_pow2_scale_rule():
    assert R.pow2_scale(None) == 1.0 and R.pow2_scale(0.0) == 1.0 and R.pow2_scale(float("inf")) == 1.0 and R.pow2_scale(float("nan")) == 1.0
    assert R.pow2_scale(1.0) == 2.0 ** 13 and R.pow2_scale(1.999) == 2.0 ** 13 and R.pow2_scale(2.0) == 2.0 ** 12 and R.pow2_scale(2049.0) == 4.0
    assert R.pow2_scale(2.0 ** -107) == 2.0 ** 120 and R.pow2_scale(2.0 ** -108) == 1.0          # exponent field 20 is the first scaled one
    assert R.pow2_scale(2.0 ** 123) == 2.0 ** -110 and R.pow2_scale(2.0 ** 124) == 1.0           # 250 the last
    for am in (0.37, 1.0, 5.5, 2049.0, 3.0e-5, 7.0e8):
        assert 2.0 ** 13 <= float(torch.tensor(am, dtype=F32)) * R.pow2_scale(am) < 2.0 ** 14


def test_split4h_follows_its_model_and_rounds_ties_to_even():
    x = R.gauss((64, 96), 3)
    am = float(x.abs().max())
    p, s = R.pieces(x, "f16x3", am)
    assert R.pieces_normal(p, "f16x3")
    e = x * s - p["h"] - p["l"] * 2.0 ** -11
    assert bool((e.abs() <= 2.0 ** -22 * (x * s).abs()).all())                           # the model of gemm_f16s.hip / split_f16.h
    assert bool((p["l"].abs() * 2.0 ** -11 <= 2.0 ** -11 * p["h"].abs()).all())
    t = torch.tensor([2049.0, 2051.0, -2049.0, 4098.0, 4102.0, 2047.0], dtype=torch.float64)
    pt, _ = R.pieces(t, "f16x3", None)                                                  # s = 1
    assert pt["h"].tolist() == [2048.0, 2052.0, -2048.0, 4096.0, 4104.0, 2047.0]
    assert pt["l"].tolist() == [2048.0, -2048.0, -2048.0, 4096.0, -4096.0, 0.0]
    tr, _ = R.pieces(t, "f16x3", None, trunc=True)
    assert tr["h"].tolist() == [2048.0, 2050.0, -2048.0, 4096.0, 4100.0, 2047.0]
    un, _ = R.pieces(t, "f16x3", None, l_unscaled=True)
    assert un["l"].tolist() == [1.0, -1.0, -1.0, 2.0, -2.0, 0.0]
    img = R.packed_image(t[:4].view(1, 4), None)
    assert img.shape == (1, 4) and img.view(torch.float16).view(-1).tolist() == [2048.0, 2052.0, -2048.0, 4096.0, 2048.0, -2048.0, -2048.0, 4096.0]


def test_split4_follows_its_model_and_rounds_ties_to_even():
    x = R.gauss((64, 96), 4)
    p, _ = R.pieces(x, "bf16x6")
    assert bool(((x - p["h"] - p["m"] - p["l"]).abs() <= 2.0 ** -24 * x.abs()).all())
    t = torch.tensor([257.0, 259.0, 65793.0, 262657.0], dtype=torch.float64)
    pt, _ = R.pieces(t, "bf16x6")
    assert pt["h"].tolist() == [256.0, 260.0, 66048.0, 262144.0] and pt["m"].tolist() == [1.0, -1.0, -255.0, 512.0] and pt["l"].tolist() == [0.0, 0.0, 0.0, 1.0]
    tr, _ = R.pieces(t, "bf16x6", trunc=True)
    assert bool((tr["h"] + tr["m"] + tr["l"] == t).all())            # three truncated pieces hold every bit of an fp32 value


def test_documented_precision_models_hold_on_the_gaussian_cases():
    """(c): |ideal - float64| <= 3 * 2^-22 sum |a||b| (f16x3, gemm_f16s.hip) and 2^-22 sum |a||b| (bf16x6, gemm_bf16s.hip)"""
    for c in (R.NT_CASES["m129_n132_k32"], R.NT_CASES["g1_d12_rect0"], R.NT_CASES["m257_n70_k288"], R.TN_CASES["k100_m64_n72"], R.TN_CASES["w_d5"], TN_ONE):
        truth = data(c, "f32", "gauss")
        for arith, bound in R.MODEL_BOUND.items():
            d = R.make_data(c, arith, "gauss")
            assert torch.equal(d["A"], truth["A"]) and torch.equal(d["B"], truth["B"])
            err, lim = (d["P"] - truth["P"]).abs(), bound * truth["Q"]
            print(f"  {arith}: max |ideal - float64| / (bound sum|a||b|) = {float((err / lim.clamp_min(1e-300)).max()):.3f}")
            assert bool((err <= lim).all()), arith
        # f16 keeps ha * hb alone: 2 * 2^-11 relative per product, far outside the f16x3 model -- the names are not interchangeable
        d = R.make_data(c, "f16", "gauss")
        assert bool(((d["P"] - truth["P"]).abs() > R.MODEL_BOUND["f16x3"] * truth["Q"]).any())


# ----------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------
def test_case_tables_reach_every_variant():
    V = {(k, p): R.variant(R.ALL_CASES[k], p) for k, p in R.runs()}
    kernels = {v["kernel"] for v in V.values()}
    for g in ("true", "false"):
        assert {f"gemm_rows_kernel<0, {g}>", f"gemm_rows_kernel<1, {g}>", f"gemm_rows_bf16s8_kernel<{g}>", f"gemm_tn_kernel<{g}>",
                f"gemm_tn_bf16s_kernel<{g}>"} <= kernels
        for np_ in (1, 3):
            for wave in ("f16s4", "f16s8"):
                for pa, pb in ((0, 0), (1, 0), (0, 1), (1, 1)):
                    assert f"gemm_rows_{wave}_kernel<{g}, {np_}, pa={pa}, pb={pb}, epi=0>" in kernels
                assert f"gemm_rows_{wave}_kernel<false, {np_}, pa=0, pb=0, epi=1>" in kernels
            assert f"gemm_tn_f16s_kernel<{g}, {np_}, pa=0, pb=0, small>" in kernels and f"gemm_tn_f16s_kernel<{g}, {np_}, pa=0, pb=0>" in kernels
            assert f"gemm_tn_f16s8_kernel<{g}, {np_}, pa=0, pb=0>" in kernels
    assert "gemm_skinny_nt_kernel" in kernels
    assert any("pa=1, pb=0" in k for k in kernels if k.startswith("gemm_tn")) and any("pa=0, pb=1" in k for k in kernels if k.startswith("gemm_tn"))
    assert any("pa=1, pb=1" in k for k in kernels if k.startswith("gemm_tn"))
    nt = {k: v for k, v in V.items() if R.ALL_CASES[k[0]]["mode"] == "nt"}
    # the host formulas, one by one
    assert all(v["skinny"] for (k, p), v in nt.items() if k.startswith("skinny")) and {R.ALL_CASES[k]["M"] for (k, p), v in nt.items() if v["skinny"]} == {1, 61}
    assert all(v["use_f16s4"] == (R.ALL_CASES[k]["K"] * R.ALL_CASES[k]["kept"] <= 256) for (k, p), v in nt.items() if "_f16s" in v["kernel"])
    for name in ("m129_n70_k33", "m127_n132_k52", "odd_lda", "base_plus_one_float"):          # every precision on the exact kernel
        assert {V[(name, p)]["kernel"] for p in R.PRECISIONS} == {"gemm_rows_kernel<0, false>"}
        assert not any(V[(name, p)]["bf16s_rows_ok"] or V[(name, p)]["f16s_rows_ok"] for p in R.PRECISIONS)
    c33 = R.NT_CASES["m129_n70_k33"]
    assert c33["lda"] % 4 == 0 and c33["K"] % 4 != 0 and V[("m129_n70_k33", "f32")]["vec_a"]       # the vector path with a K tail
    assert not V[("odd_lda", "f32")]["vec_a"] and not V[("base_plus_one_float", "f32")]["vec_a"]
    assert {v["wide_store"] for v in nt.values() if "wide_store" in v} == {True, False}
    cs = list(R.NT_CASES.values())
    assert {129, 257, 127, 255} <= {c["M"] for c in cs} and {132, 70, 4} <= {c["N"] for c in cs} and {32, 288, 33, 52} <= {c["K"] for c in cs}
    assert any(c["batch"] == 3 and c["bsa"] > c["rows_a"] * c["lda"] for c in cs) and any(c["alpha"] == 0.5 and c["bias"] for c in cs)
    assert all(c["lda"] > c["K"] and c["ldb"] > c["K"] and c["ldc"] > c["N"] for c in cs)
    for g in (1, 2):
        assert {c["conv"][4] for c in cs if c["gather"] == g and c["rect"] == 0} >= {1, 2}
        for dil in (12, 24):
            assert {c["rect"] for c in cs if c["gather"] == g and c["conv"][6] == dil} >= {1, 2}
        assert any(c["gather"] == g and c["tap_mask"] is not None and R.popcount(c["mask"]) < 9 for c in cs)
    assert {c["rect"] for c in cs if c["gather"] == 1 and c["conv"][6] in (12, 24)} == {0, 1, 2}
    epi = [c for c in cs if c["epi"] is not None]
    assert {c["epi"][1] for c in epi} == {True, False} and all(c["epi"][0] != c["ldc"] for c in epi) and any(c["epi"][0] for c in epi)
    nn = list(R.NN_CASES.values())
    assert any(c["gather"] for c in nn) and any(c["rect"] == 1 for c in nn) and any(c["batch"] == 3 and c["bias"] and c["accumulate"] and c["alpha"] != 1 for c in nn)
    assert all(V[(k, p)]["kernel"].startswith("gemm_rows_kernel<1") for k in R.NN_CASES for p in R.NN_CASES[k]["precs"])
    tn = {k: v for k, v in V.items() if R.ALL_CASES[k[0]]["mode"] == "tn"}
    assert {v["lanes"] for v in tn.values()} == {0, 1, 4, 16} and any(v["empty_slices"] for v in tn.values())
    assert any(v["second_vec"] is False for v in tn.values()) and {v.get("second") for v in tn.values()} >= {"tn_reduce_kernel", "tn_reduce_lanes_kernel", "tn_reduce_oihw_kernel"}
    assert V[("k40_m64_n72_s3_empty", "f32")]["empty_slices"] == 1 and V[("k300_m132_n72_s9", "f32")]["lanes"] == 4 and V[("k1056_m64_n72_s33", "f32")]["lanes"] == 16
    assert all(V[("k100_m66_n72_exact", p)]["kernel"] == "gemm_tn_kernel<false>" for p in R.PRECISIONS)
    ts = list(R.TN_CASES.values())
    assert all(c["lda"] > c["M"] and c["ldb"] > c["N"] for c in ts) and any(c["batch"] == 3 for c in ts) and any(c["accumulate"] for c in ts)
    assert {(c["conv"][4], c["conv"][6]) for c in ts if c["conv"]} >= {(1, 1), (2, 1), (1, 5)} and {c["rect"] for c in ts if c["conv"]} == {0, 1}
    assert any(c["oihw"] and c["foreign"] is None for c in ts) and any(c["oihw"] and c["foreign"] is not None and not (c["mask"] >> c["foreign"]) & 1 for c in ts)
    assert max(max(c["M"], c["rows_a"] if c["mode"] != "tn" else c["K"]) for c in R.ALL_CASES.values()) <= 3025 and max(c["N"] for c in R.ALL_CASES.values()) <= 264


def test_every_run_meets_the_preconditions_of_its_gate():
    """make_data asserts them: integer families -- sum |terms| / unit < 2^24 and an fp32 reference; Gaussians -- every scaled fp16
    piece zero or normal"""
    seen, worst = set(), 0.0
    for name, prec in R.runs():
        c = R.ALL_CASES[name]
        arith = R.variant(c, prec)["arith"]
        for family in R.families_of(arith):
            if (name, arith, family) not in seen:
                seen.add((name, arith, family))
                d = R.make_data(c, arith, family)
                if d["exact"]:
                    worst = max(worst, float(d["ratio"].max()))
                    assert float(d["ref"].abs().max()) > 0
    print(f"  {len(seen)} (case, arithmetic, family) combinations; largest sum |terms| / unit = 2^{torch.tensor(worst).log2():.2f}")
    for prec in R.SPLIT16:
        d = R.make_data(R.SUBNORMAL_CASE, prec, "gauss", subnormal=True)
        lo = min(float(d[k][d[k] != 0].abs().min()) / float(d[k].abs().max()) for k in ("A", "B"))
        assert 2.0 ** -27 <= lo < 2.0 ** -24 and float(d["extra"].min()) > 0


def test_integer_families_light_every_kept_product_and_no_dropped_one():
    for c in (R.NT_CASES["m129_n132_k32"], R.NT_CASES["g1_s1"], R.TN_CASES["k100_m64_n72"]):
        for arith in ("bf16x6", "f16x3", "f16"):
            kept = {(a, b) for a, b, _ in R.PRODUCTS[arith]}
            lit = {}
            for family in R.FAMILIES[arith]:
                cov = R.piece_coverage(c, arith, family)
                dropped = {k: v for k, v in cov.items() if k not in kept and v > 0}
                assert (family == "i13" and set(dropped) == {("l", "h")}) or not dropped, (arith, family, dropped)
                for k in kept:
                    lit[k] = max(lit.get(k, 0.0), cov[k])
            assert all(v > 0 for v in lit.values()) and set(lit) == kept, (arith, lit)


# ----------------------------------------------------------------------------------------
# acceptance: the ideal result in fp32, in a shuffled order
# ----------------------------------------------------------------------------------------
def shuffled_fp32(c, d, arith, seed):
    """every kept piece product of every k of an NT case as its own fp32 term (exact: 8 x 8 and 11 x 11 bits; f32: rounded once),
    summed in fp32 in a random order, then alpha / bias in fp32 as the epilogue does"""
    A, B = d["A"][0], d["B"][0][0]
    pa, sa = R.pieces(A, arith, d["amax_a"])
    pb, sb = R.pieces(B, arith, d["amax_b"])
    terms = torch.cat([(w * pa[na][:, None, :] * pb[nb][None, :, :]).float() for na, nb, w in R.PRODUCTS[arith]], -1)       # [M][N][P K]
    order = torch.randperm(terms.shape[-1], generator=torch.Generator().manual_seed(seed))
    acc = torch.zeros(terms.shape[:2], dtype=F32)
    for i in order.tolist():
        acc = acc + terms[:, :, i]
    v = acc * torch.tensor(d["alpha"] / (sa * sb), dtype=F32)
    return (v + d["bias"].float()).view(1, *v.shape)


@pytest.mark.parametrize("arith", R.PRECISIONS)
def test_gates_accept_the_ideal_result_summed_in_fp32_in_a_shuffled_order(arith):
    for family in R.families_of(arith):
        d = data(NT_SMALL, arith, family)
        for seed in (1, 2):
            got = shuffled_fp32(NT_SMALL, d, arith, seed)
            assert not rejected(got, d), (arith, family)
            if not d["exact"]:
                worst = R.gate_interval(got, d["ref"], d["absref"], d["n_terms"], f"shuffled {arith}")
                assert worst < 0.25                                     # a random order stays far inside the worst-case bound
            assert not rejected(evaluate(NT_SMALL, d, arith), d)


# ----------------------------------------------------------------------------------------
# mutants
# ----------------------------------------------------------------------------------------
def _gauss_case_for(arith, product):
    """dropping one of the three lowest bf16x6 products moves an element by about 2^-17 of one term: visible to a worst-case
    accumulation bound only where the reduction is a few terms long"""
    return TN_ONE if (arith == "bf16x6" and product in (("l", "h"), ("m", "m"), ("h", "l"))) else NT_SMALL


@pytest.mark.parametrize("arith", ["bf16x6", "f16x3"])
def test_each_single_kept_product_dropped_is_rejected(arith):
    for na, nb, _ in R.PRODUCTS[arith]:
        hit = 0
        for family in R.FAMILIES[arith]:                                 # every integer family that lights the product rejects
            d = data(NT_SMALL, arith, family)
            if R.piece_coverage(NT_SMALL, arith, family)[(na, nb)] > 0:
                assert rejected(evaluate(NT_SMALL, d, arith, drop=(na, nb)), d), (arith, family, na, nb)
                hit += 1
        assert hit >= 1
        c = _gauss_case_for(arith, (na, nb))
        d = data(c, arith, "gauss")
        assert rejected(evaluate(c, d, arith, drop=(na, nb)), d), (arith, "gauss", na, nb)


def test_tightness_the_interval_rejects_what_the_old_gate_accepts():
    d = data(TN_ONE, "bf16x6", "gauss")
    assert not rejected(evaluate(TN_ONE, d, "bf16x6"), d) and R.close_old(evaluate(TN_ONE, d, "bf16x6"), d["ref"])
    for drop in (("l", "h"), ("m", "m"), ("h", "l")):
        got = evaluate(TN_ONE, d, "bf16x6", drop=drop)
        bad, worst = R.interval_violations(got, d["ref"], d["absref"], d["n_terms"], False)
        print(f"  bf16x6 without {drop[0]}a*{drop[1]}b: {int(bad.sum())} of {got.numel()} elements outside the interval, worst {worst:.1f} d; "
              f"close(5e-5) accepts: {R.close_old(got, d['ref'])}")
        assert int(bad.sum()) > 0.05 * got.numel() and R.close_old(got, d["ref"])
    # the same at the NT kernels' shortest reduction, K = 32, against the old gate's operands (uniform in [-1, 1]): accepted
    g = torch.Generator().manual_seed(3)
    A, B = (torch.rand(1, 33, 33, generator=g) * 2 - 1).double(), (torch.rand(1, 1, 20, 33, generator=g) * 2 - 1).double()
    src = torch.arange(33).view(1, -1)
    full = R.ideal("nt", A[0], B[0], src, 1, "bf16x6")[0]
    for drop in (("l", "h"), ("m", "m"), ("h", "l")):
        assert R.close_old(R.ideal("nt", A[0], B[0], src, 1, "bf16x6", drop=drop)[0].float(), full)


def test_low_piece_without_its_scaling_and_a_truncating_split_are_rejected():
    for family in R.FAMILIES["f16x3"]:
        d = data(NT_SMALL, "f16x3", family)
        assert rejected(evaluate(NT_SMALL, d, "f16x3", l_unscaled=True), d), family
    d = data(NT_SMALL, "f16x3", "gauss")
    assert rejected(evaluate(NT_SMALL, d, "f16x3", l_unscaled=True), d)
    # truncation.  Integers: the i13 family under f16 (under f16x3 and bf16x6 an exact split of an exactly summable operand gives
    # the same sum however it rounds).  Gaussians: f16 at K = 32; f16x3 at one reduction row (|e| <= 2^-20 |x s|, one-sided)
    d = data(NT_SMALL, "f16", "i13")
    assert rejected(evaluate(NT_SMALL, d, "f16", trunc=True), d)
    d = data(NT_SMALL, "f16", "gauss")
    assert rejected(evaluate(NT_SMALL, d, "f16", trunc=True), d)
    d = data(TN_ONE, "f16x3", "gauss")
    assert rejected(evaluate(TN_ONE, d, "f16x3", trunc=True), d)


@pytest.mark.parametrize("arith", R.PRECISIONS)
def test_dropped_k_step_tap_and_padding_column_are_rejected(arith):
    for family in R.families_of(arith):
        d = data(NT_SMALL, arith, family)
        A = d["A"].clone()
        A[:, :, 16:32] = 0.0                                             # one 16-deep k-step
        assert rejected(evaluate(NT_SMALL, d, arith, A=A), d), (arith, family, "k-step")
        # one padding column of A (and the B column it would meet) in the sum: what a float4 load past K lets in
        pad_a, pad_b = d["A"][:, :, :1].abs().clamp_min(1.0), d["B"][..., :1].abs().clamp_min(1.0)
        got = evaluate(NT_SMALL, d, arith, A=torch.cat([d["A"], pad_a], -1), B=torch.cat([d["B"], pad_b], -1))
        assert rejected(got, d), (arith, family, "padding column")
        g = data(NT_GATHER, arith, family)
        assert not rejected(evaluate(NT_GATHER, g, arith), g)
        for tap in (0, 4, 8):
            assert rejected(evaluate(NT_GATHER, g, arith, mask=g["mask"] & ~(1 << tap)), g), (arith, family, "tap", tap)


@pytest.mark.parametrize("arith", R.PRECISIONS)
def test_one_element_two_ulp_off(arith):
    for family in R.families_of(arith):
        d = data(NT_SMALL, arith, family)
        got = evaluate(NT_SMALL, d, arith)
        i = (0,) + tuple(int(v) for v in got[0].abs().argmax().unsqueeze(0).div(got.shape[2], rounding_mode="floor").tolist()) + (int(got[0].abs().argmax()) % got.shape[2],)
        off = got.clone()
        off[i] = (off[i].view(torch.int32) + 2).view(F32)
        assert float(off[i]) != float(got[i])
        if d["exact"]:
            assert rejected(off, d), (arith, family)
        else:
            # 2 ulp of the result <= 2 * 2^-23 absref < (P n + 4) 2^-23 absref: inside any accumulation bound, by derivation
            assert not rejected(off, d)


def test_frame_detects_a_store_outside_the_logical_c():
    f = R.Frame((2, 3, 5), (40, 8, 1), F32, off=16, tail=88)
    f.put(torch.ones(2, 3, 5))
    f.dev = f.host.clone()
    assert torch.equal(f.result(), torch.ones(2, 3, 5))
    for where in (16 + 5, 16 + 40 + 2 * 8 + 5, 15, 16 + 3 * 8):          # padding column, behind the last element, in front, the row behind batch 0
        f.dev = f.host.clone()
        f.dev[where] = 0.0
        with pytest.raises(AssertionError, match="outside the logical tensor"):
            f.result()


def test_split_probe_has_ties_zeros_the_maximum_and_normal_pieces():
    x, settings = R.split_probe()
    assert settings[0] == float(x.abs().max()) and settings[1] == 8 * settings[0] and settings[2] == 0.0
    assert [R.pow2_scale(s) for s in settings][2] == 1.0 and R.pow2_scale(settings[0]) == 8 * R.pow2_scale(settings[1])
    for am in settings:
        p, s = R.pieces(x, "f16x3", am)
        assert R.pieces_normal(p, "f16x3") and bool((p["l"] != 0).any())
        img = R.packed_image(x, am).view(torch.float16).view(x.shape[0], -1, 8)
        assert torch.equal(img[..., :4].reshape(x.shape).double(), p["h"]) and torch.equal(img[..., 4:].reshape(x.shape).double(), p["l"])
