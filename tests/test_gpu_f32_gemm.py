"""GPU: the fp32-storage contraction kernels (csrc/gemm_f32.hip, gemm_bf16s.hip, gemm_f16s.hip, gemm_f16s4.hip with
gemm_rows_walk.h and gemm_tn_walk.h) driven through ops.gemm -- and glf_amax / glf_split_f16_packed(_colsum) through _lib -- under
the f32, bf16x6, f16x3 and f16 precisions, judged element by element against the float64 ideal result of the precision
(tests/f32_gemm_ref.py states the reference, the operand families, the two gates and their derivation; tests/
test_f32_gemm_ref_cpu.py proves on the CPU that they reject a dropped product, a truncating split, a dropped k-step or tap, a
padding column in the sum, a 2-ulp error and a store outside C).

Every operand and C is a view into a larger NaN-filled buffer (S16.Frame): row strides larger than the logical width (lda > K,
ldb > K, ldc > N; TN lda > M, ldb > N), NaN rows behind the last logical row, gaps between batches and taps, offsets multiples of
4 floats for the aligned paths; two deliberately misaligned layouts (an odd lda, a base pointer one float off) send every
precision to the exact-fp32 kernel.  After each call every logical C element is finite and the bit pattern of every C-buffer
element outside the logical C is unchanged.  The kernel a case reaches (host formulas of the launchers) is printed with the
case, and the last test prints, per kernel and precision, the worst |got - ideal| / d over its Gaussian runs and the number of
differing elements over its integer runs.

Out of scope: the segmented region mode (nseg, glf_gemm_nt_seg_cols) and the colstats / colmax sums have their own tests
(test_gpu_aspp_fwd_one.py, test_gpu_aspp_dgrad_one.py, test_gpu_rows_walk.py, test_gpu_bn_stream.py)."""
import pytest
import torch

import f32_gemm_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = torch.float32
REPORT = {}                      # (kernel, precision) -> [runs, worst Gaussian ratio, differing integer elements]


@pytest.fixture(autouse=True)
def _restore_precision():
    yield
    if torch.cuda.is_available():
        from glfusion_amd import ops
        ops.set_precision("f32")


def _frame(dims, strides, off=16):
    ld = max(int(s) for s in strides)
    return R.Frame(dims, strides, F32, off=off, tail=2 * ld + 72)


def _scalar(v):
    return None if v is None else torch.tensor([v], dtype=F32, device=DEV)


def _operand(x, packed, amax):
    """the fp32 operand, or its packed pre-split image (built on the host; test_split_images_* pin the device's to the same bits)"""
    return R.packed_image(x, amax) if packed else x.float()


def _record(v, prec, ratio=None, ndiff=None):
    r = REPORT.setdefault((v["kernel"], prec), [0, 0.0, 0])
    r[0] += 1
    if ratio is not None:
        r[1] = max(r[1], ratio)
    if ndiff is not None:
        r[2] += ndiff


def _judge(got, d, v, prec, what, record=True):
    assert bool(torch.isfinite(got).all()), what + ": non-finite element in the logical C"
    if not record:
        R.gate_interval(got, d["ref"], d["absref"], d["n_terms"], what, extra=d["extra"])
    elif d["exact"]:
        ndiff = int((got.double() != d["ref"]).sum())
        _record(v, prec, ndiff=ndiff)
        R.gate_exact(got, d["ref"], False, what)
    else:
        ratio = R.gate_interval(got, d["ref"], d["absref"], d["n_terms"], what, extra=d["extra"])
        _record(v, prec, ratio=ratio)


def run_rows(name, c, prec, subnormal=False, judge_as=None):
    """judge_as: the Gaussian run alone, judged against the ideal of ANOTHER precision (which must fail: see the last tests)"""
    from glfusion_amd import ops
    v = R.variant(c, prec)
    arith = judge_as or v["arith"]
    M, N, K, batch, taps = c["M"], c["N"], c["K"], c["batch"], c["taps"]
    print(f"\n  {c['mode'].upper()} {name} [{prec}] M {M} N {N} K {K} batch {batch} gather {c['gather']} conv {c['conv']} rect {c['rect']} "
          f"mask {c['mask']:#x}: {v}")
    ops.set_precision(prec)
    for family in (("gauss",) if (subnormal or judge_as) else R.families_of(arith)):
        d = R.make_data(c, arith, family, subnormal=subnormal)
        what = f"{name} [{prec}] {family}"
        dA = _frame((batch, c["rows_a"], K), (c["bsa"], c["lda"], 1), off=c["a_off"]).put(_operand(d["A"], c["pa"], d["amax_a"])).upload()
        dB = _frame((batch, taps) + c["b_dims"], (c["bsb"], c["tsb"], c["ldb"], 1), off=c["b_off"]).put(_operand(d["B"], c["pb"], d["amax_b"])).upload()
        dbias = _frame((N,), (1,), off=4).put(d["bias"].float()).upload() if d["bias"] is not None else None
        fc = _frame((batch, M, N), (c["bsc"], c["ldc"], 1), off=c["c_off"])
        if d["cold"] is not None:
            fc.put(d["cold"].float())
        elif c["rect"] == 1:
            fc.put(torch.zeros(batch, M, N))                     # per-tap rectangles meet in float atomics: a zero-filled C
        epilogue = None
        if c["epi"] is not None:
            ld_res, relu = c["epi"]
            dres = _frame((M, N), (ld_res, 1)).put(d["res"][0].float()).upload() if ld_res is not None else None
            epilogue = (dres, ld_res or 0, relu)
        given = c["amax"] != "self" and arith in ("f16x3", "f16")
        slot = torch.zeros(1, dtype=F32, device=DEV) if c["amax_c"] else None
        ops.gemm(c["mode"], dA, dB, fc.upload(), M=M, N=N, K=K, lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], bias=dbias, taps=taps, mask=c["mask"],
                 tap_stride_b=c["tsb"], gather=c["gather"], geo=c["geo"], batch=batch, bsa=c["bsa"], bsb=c["bsb"], bsc=c["bsc"], alpha=d["alpha"],
                 accumulate=c["accumulate"], rect=c["rect"], amax_a=_scalar(d["amax_a"]) if given else None,
                 amax_b=_scalar(d["amax_b"]) if given else None, amax_c=slot, a_packed=c["pa"], b_packed=c["pb"], epilogue=epilogue)
        torch.cuda.synchronize()
        got = fc.result(what)
        _judge(got, d, v, prec, what, record=judge_as is None)
        if slot is not None and (v["skinny"] or arith in ("f16x3", "f16")):
            assert float(slot) == float(got.abs().max()), f"{what}: amax_c {float(slot)} is not max |C| {float(got.abs().max())}"


def run_tn(name, c, prec):
    from glfusion_amd import ops
    v = R.variant(c, prec)
    arith = v["arith"]
    M, N, K, batch, taps, live = c["M"], c["N"], c["K"], c["batch"], c["taps"], R.kept_taps(c["mask"], c["taps"])
    print(f"\n  TN {name} [{prec}] K {K} M {M} N {N} batch {batch} split {c['split']} conv {c['conv']} rect {c['rect']} mask {c['mask']:#x} "
          f"oihw {c['oihw']}: {v}")
    ops.set_precision(prec)
    for family in R.families_of(arith):
        d = R.make_data(c, arith, family)
        what = f"{name} [{prec}] {family}"
        dA = _frame((batch, K, M), (c["bsa"], c["lda"], 1)).put(_operand(d["A"], c["pa"], d["amax_a"])).upload()
        dB = _frame((batch, c["rows_b"], N), (c["bsb"], c["ldb"], 1)).put(_operand(d["B"], c["pb"], d["amax_b"])).upload()
        foreign = None
        if c["oihw"]:
            fc = _frame((M, N, taps), (N * taps, taps, 1))
            if d["cold"] is not None:
                fc.put(d["cold"][0].permute(1, 2, 0).float())
            if c["foreign"] is not None:
                foreign = (c["foreign"], _frame((M, N), (N + 4, 1)).put(d["foreign"].float()).upload(), N + 4)
            ref, absref = d["ref"], d["absref"]
        else:
            # only the slabs of the kept taps are logical C: those of the masked-out taps must stay untouched
            fc = _frame((batch, taps, M, N), (c["bsc"], c["tsb"], c["ldc"], 1))
            fc.idx = fc.idx[:, live]
            if d["cold"] is not None:
                fc.put(d["cold"][:, live].float())
            ref, absref = d["ref"][:, live], d["absref"][:, live]
        given = c["amax"] != "self" and arith in ("f16x3", "f16")
        ops.gemm("tn", dA, dB, fc.upload(), M=M, N=N, K=K, lda=c["lda"], ldb=c["ldb"], ldc=c["ldc"], taps=taps, mask=c["mask"], tap_stride_b=c["tsb"],
                 gather=c["gather"], geo=c["geo"], batch=batch, bsa=c["bsa"], bsb=c["bsb"], bsc=c["bsc"], alpha=d["alpha"], accumulate=c["accumulate"],
                 split=c["split"], rect=c["rect"], amax_a=_scalar(d["amax_a"]) if given else None, amax_b=_scalar(d["amax_b"]) if given else None,
                 a_packed=c["pa"], b_packed=c["pb"], oihw=c["oihw"], foreign=foreign)
        torch.cuda.synchronize()
        got = fc.result(what)
        if c["oihw"]:
            got = got.permute(2, 0, 1).unsqueeze(0)
        _judge(got, dict(d, ref=ref, absref=absref), v, prec, what)


@pytest.mark.parametrize("name,prec", R.runs(R.NT_CASES))
def test_nt(name, prec):
    run_rows(name, R.NT_CASES[name], prec)


@pytest.mark.parametrize("name,prec", R.runs(R.NN_CASES))
def test_nn(name, prec):
    run_rows(name, R.NN_CASES[name], prec)


@pytest.mark.parametrize("name,prec", R.runs(R.TN_CASES))
def test_tn(name, prec):
    run_tn(name, R.TN_CASES[name], prec)


@pytest.mark.parametrize("prec", R.SPLIT16)
def test_nt_elements_down_to_2_pow_minus_27_of_the_maximum(prec):
    """h stays normal, l may be subnormal: the bound gains one fp16 subnormal spacing per operand and term (2^-24 / s), which
    covers gradual underflow and a flush to zero of the low piece alike"""
    run_rows("subnormal", R.SUBNORMAL_CASE, prec, subnormal=True)


# ----------------------------------------------------------------------------------------
# the packed pre-split images and glf_amax against the host emulation, bit for bit
# ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("colsum", [False, True])
def test_split_images_equal_the_host_emulation_bitwise(colsum):
    from glfusion_amd._lib import lib
    rows, cols, ld, ldo = 37, 72, 80, 84
    x, settings = R.split_probe(rows, cols)
    dx = _frame((rows, cols), (ld, 1)).put(x.float()).upload()
    got_max = torch.full((1,), -1.0, dtype=F32, device=DEV)
    assert lib.glf_amax(dx.data_ptr(), rows, cols, ld, got_max.data_ptr(), None) == 0, lib.glf_last_error()
    torch.cuda.synchronize()
    assert float(got_max) == settings[0] == float(x.abs().max())
    for am in settings:
        want = R.packed_image(x, am)
        fo = _frame((rows, cols), (ldo, 1))
        damax = _scalar(am)
        if colsum:
            sums = torch.full((cols + 16,), float("nan"), dtype=F32, device=DEV)
            ws = torch.empty(int(lib.glf_bn_workspace(rows, cols)), dtype=torch.float64, device=DEV)
            rc = lib.glf_split_f16_packed_colsum(dx.data_ptr(), rows, cols, ld, damax.data_ptr(), fo.upload().data_ptr(), ldo, sums.data_ptr(),
                                                 ws.data_ptr(), None)
        else:
            rc = lib.glf_split_f16_packed(dx.data_ptr(), rows, cols, ld, damax.data_ptr(), fo.upload().data_ptr(), ldo, None)
        assert rc == 0, lib.glf_last_error()
        torch.cuda.synchronize()
        got = fo.result(f"packed image (amax {am})")
        bad = got.view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), (f"amax {am} (s = {R.pow2_scale(am)}): {int(bad.sum())} of {got.numel()} words differ from the host split4h; first at "
                                     f"{tuple(int(i) for i in bad.nonzero()[0])}")
        if colsum:
            assert bool(torch.isnan(sums[cols:]).all()), "a write landed behind colsum"
            ref = x.sum(0)
            assert bool(((sums[:cols].cpu().double() - ref).abs() <= (rows + 4) * 2.0 ** -23 * x.abs().sum(0)).all())


@pytest.mark.parametrize("name", ["m129_n132_k32", "m129_n70_k32_b3"])
@pytest.mark.parametrize("prec,other", [("f16", "f16x3"), ("f16x3", "f16")])
def test_the_interval_tells_f16_from_f16x3_on_the_device(name, prec, other):
    """the two precisions share kernels, operands and scales and differ in two MFMAs per product: a kernel launched as one of them
    and judged as the other leaves the interval (the whole-tensor gates of test_gpu_ops.py give f16 2e-2).  At K = 32, where the
    bound, which grows with K, is still below the 2^-12 per product that separates the two."""
    with pytest.raises(AssertionError, match="outside the derived interval"):
        run_rows(name, R.NT_CASES[name], prec, judge_as=other)


def test_zz_report():
    """per kernel and precision: runs, the worst |got - ideal| / d of the Gaussian runs (<= 1), differing integer elements (0)"""
    print("\n  kernel | precision | runs | worst |got - ideal| / d | differing integer elements")
    for (kernel, prec), (n, worst, ndiff) in sorted(REPORT.items()):
        print(f"  {kernel} | {prec} | {n} | {worst:.3f} | {ndiff}")
    assert all(worst <= 1.0 and ndiff == 0 for _, worst, ndiff in REPORT.values())
