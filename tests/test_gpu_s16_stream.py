"""GPU: the 16-bit-storage streaming kernels (csrc/norm.hip, csrc/s16_ops.hip) called through their C entry points and judged element by element
against float64 on the same bf16 inputs, every output in a guarded buffer: glf_s16_colstats, glf_s16_colsum, glf_s16_bn_apply (train
and eval), glf_s16_bn_bwd (all six reduce instantiations x training x dres), glf_s16_bn_res_ln_fwd / _bwd, glf_s16_sum_rows,
glf_s16_cast, and their refusals.

Integer inputs are gated for equality, Gaussian ones by the interval d = (k + 4) 2^-23 magnitude with k counted from the kernel
source: the derivation of every k, the input families and the treatment of ReLU signs are in tests/s16_stream_ref.py; its CPU
side (references against torch, preconditions at every shape used here, the gates' teeth) is tests/test_s16_stream_ref_cpu.py.
A statistic the kernel writes (mean, invstd, row_mean, row_rstd, dbeta, dgamma) is gated against float64 first; the outputs that
depend on it then take the value the kernel wrote, so neither error is charged to the other.  Accumulation buffers (`sums`) start
from a known content, so `written()` means: compared in full.  The largest |got - ref| / d per output is printed when the module
finishes (recorded in profiles/s16_stream_gate.txt)."""
import functools

import pytest
import torch

import s16_stream_ref as R
from s16_stream_ref import BF, DEV, F32, F64, Guarded, Guarded16, gate, exact, ptr, put16, vec32

pytestmark = pytest.mark.gpu

OK, ERR_BAD_SHAPE, ERR_UNSUPPORTED, ERR_NULL = 0, -1, -2, -5      # include/glfusion.h
DT_F32, DT_BF16 = 0, 1
FAMILIES = ["int", "gauss"]
COMBOS = ((False, False, False), (False, True, False), (True, True, True), (True, False, False), (False, True, True))   # residual, relu, mask


@pytest.fixture(scope="module")
def L():
    from glfusion_amd._lib import lib, check
    yield lib, check
    for name, (n, worst, off) in sorted(R.RATIOS.items()):
        print(f"\nS16_STREAM_GATE {name}: tensors {n}, max |got - ref| / d {worst:.4g}, largest share != bf16_rne(ref) {off:.3g}", end="")
    print(f"\nS16_STREAM_GATE train-mode dx, mask bytes against recomputed signs: bitwise check skipped {SKIPPED_ROUTE_CHECKS[0]}, made {SKIPPED_ROUTE_CHECKS[1]}")


def sync():
    torch.cuda.synchronize()


def guards(*bufs, what=""):
    for g in bufs:
        if g is not None:
            assert g.intact(), f"{what}: a guard element or a pad column was overwritten"
            assert g.written(), f"{what}: an element was not written"


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16 if a.dtype == BF else torch.int32), b.contiguous().view(torch.int16 if b.dtype == BF else torch.int32))


# ------------------------------------------------------------------------------------------------------ column reductions
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("rows,c", R.BN_SHAPES + [(5, 4104), (297, 4104), (1031, 4104)])
def test_colstats_and_colsum(L, rows, c, pad):
    lib, check = L
    k = R.red_geometry(rows, c)[4]
    for fam in FAMILIES:
        I = R.bn_inputs(fam, rows, c)
        xb, dyb = put16(I.x, c + pad), put16(I.dy, c + pad)
        ref, mag = R.colstats_ref(I.x)
        start = R.ints((2, c), 61, 1, 9).to(DEV) if pad else torch.zeros(2, c, dtype=F64, device=DEV)     # it adds to what is there
        sums = Guarded(2, c, dtype=F64).fill(start)
        check(lib.glf_s16_colstats(ptr(xb), c + pad, rows, c, sums.ptr, None), "s16_colstats")
        dref, dmag = I.dy.sum(0, keepdim=True), I.dy.abs().sum(0, keepdim=True)
        db, ws = Guarded(1, c), Guarded(1, 2 * c, dtype=F64)
        check(lib.glf_s16_colsum(ptr(dyb), c + pad, db.ptr, rows, c, ws.ptr, None), "s16_colsum")
        sync()
        guards(sums, db, ws, what=f"{fam} colstats / colsum")
        what = f"{fam} {rows} x {c} pad {pad}"
        if fam == "int":
            R.assert_exact(mag, dmag)
            exact(sums.f64(), start + ref, False, what + " colstats", "colstats sums")
            exact(db.t, dref, False, what + " colsum", "colsum db")
        else:
            gate(sums.f64() - start, ref, mag, k, False, what + " colstats", "colstats sums")
            gate(db.t, dref, dmag, k + 1, False, what + " colsum", "colsum db")


# --------------------------------------------------------------------------------------------------------- BatchNorm apply
@pytest.mark.parametrize("pads", list(R.APPLY_PADS))
@pytest.mark.parametrize("rows,c", R.BN_SHAPES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_bn_apply_train_and_eval(L, fam, rows, c, pads):
    lib, check = L
    px, pr, py = R.APPLY_PADS[pads]
    I = R.bn_inputs(fam, rows, c)
    xb, rb = put16(I.x, c + px), put16(I.res, c + pr)
    gamma, beta = vec32(I.gamma), vec32(I.beta)
    sums = R.colstats_ref(I.x)[0].contiguous()                  # in float64, from the input
    m64, is64, unb = R.bn_stats_from_sums(sums, rows)
    rm0, rv0 = R.uniform32((c,), 51, -0.1, 0.1).to(DEV), R.uniform32((c,), 52, 0.5, 1.5).to(DEV)
    nbt = torch.tensor([R.SENT_I, 0, R.SENT_I], dtype=torch.int64, device=DEV)
    calls = 0
    for train in (True, False):
        # batch statistics of five small integers are small rationals (invstd = 0.625, ...) under which BN(x) + beta lands within 1e-6
        # of zero: the integer family is built for GIVEN statistics.  In train mode it still runs -- statistics, running statistics,
        # the y interval (valid on every element) and mask bytes against the y written -- without the one comparison that needs
        # sure signs, mask bytes against float64, and so without the cap
        signs64 = train is False or fam == "gauss"
        pre_mean, pre_is = (m64.float().double(), is64.float().double()) if train else (I.mean, I.invstd)
        for res in (None, I.res) if signs64 else ():             # the cap, from the reference alone
            v, mag = R.bn_fwd_ref(I.x, pre_mean, pre_is, I.gamma, I.beta, res)
            assert R.unsure_share(R.unsure_of(v, mag, R.K_Y)) <= R.UNSURE_CAP
        for res, relu, want_mask in COMBOS:
            what = f"{fam} {rows} x {c} {pads} {'train' if train else 'eval'} res {res} relu {relu} mask {want_mask}"
            y = Guarded16(rows, c, c + py)
            mask = Guarded(1, rows * (c // 8), dtype=torch.uint8) if want_mask else None
            mo, io = Guarded(1, c), Guarded(1, c)
            if train:
                rm, rv = Guarded(1, c).fill(rm0), Guarded(1, c).fill(rv0)
                check(lib.glf_s16_bn_apply(ptr(xb), c + px, ptr(rb) if res else None, c + pr, y.ptr, c + py, ptr(sums), rows, c, R.EPS, R.MOM,
                                           ptr(gamma), ptr(beta), mo.ptr, io.ptr, rm.ptr, rv.ptr, nbt[1:].data_ptr(), int(relu), ptr(mask), None),
                      "s16_bn_apply")
                calls += 1
                sync()
                guards(mo, io, rm, rv, what=what)
                assert R.within_ulps(mo.t[0], m64) and R.within_ulps(io.t[0], is64), what + ": mean / invstd beyond one fp32 ulp"
                assert R.close(rm.t[0], (1 - R.MOM) * rm0 + R.MOM * m64, 1e-6), what + ": running_mean"
                assert R.close(rv.t[0], (1 - R.MOM) * rv0 + R.MOM * unb, 1e-5), what + ": running_var"
            else:
                mo.fill(I.mean)
                io.fill(I.invstd)
                keep = (mo.buf.clone(), io.buf.clone())
                check(lib.glf_s16_bn_apply(ptr(xb), c + px, ptr(rb) if res else None, c + pr, y.ptr, c + py, None, rows, c, R.EPS, R.MOM,
                                           ptr(gamma), ptr(beta), mo.ptr, io.ptr, None, None, nbt[1:].data_ptr(), int(relu), ptr(mask), None),
                      "s16_bn_apply(eval)")
                sync()
                assert torch.equal(mo.buf, keep[0]) and torch.equal(io.buf, keep[1]), what + ": eval mode touched mean / invstd"
            assert nbt.tolist() == [R.SENT_I, calls, R.SENT_I], what + ": num_batches_tracked must advance by one per training call"
            guards(y, what=what)
            mean, invstd = mo.f64()[0], io.f64()[0]             # what the kernel used
            v, mag = R.bn_fwd_ref(I.x, mean, invstd, I.gamma, I.beta, I.res if res else None)
            # relu is 1-Lipschitz: the interval around relu(v) holds on unsure elements as well
            gate(y.f64(), torch.relu(v) if relu else v, mag, R.K_Y, True, what, "bn_apply y")
            if mask is not None:
                got = mask.t.view(rows, c // 8)
                of_y = R.sign_bytes(y.f64() > 0)
                assert mask.intact() and mask.written(allow=(of_y == R.SENT_B).view(1, -1)), what + ": mask guard / unwritten byte"
                assert torch.equal(got, of_y), what + ": mask bytes disagree with the y written"
                sure = ~R.unsure_of(v, mag, R.K_Y)
                assert not signs64 or torch.equal(got & R.sign_bytes(sure), R.sign_bytes((v > 0) & sure)), what + ": mask bytes disagree with float64"


# ------------------------------------------------------------------------------------------------------ BatchNorm backward
def _bwd_call(lib, check, B, has2, rm, training, want_dres, mask_bytes):
    rows, c = B.rows, B.c
    pdy, pdy2, px, pdx, pdres = B.pads
    dx, dres = Guarded16(rows, c, c + pdx), (Guarded16(rows, c, c + pdres) if want_dres else None)
    dg, db = Guarded(1, c), Guarded(1, c)
    sums = Guarded(1, 2 * c, dtype=F64).fill(torch.zeros(1, 2 * c))
    check(lib.glf_s16_bn_bwd(ptr(B.dyb), c + pdy, ptr(B.dy2b) if has2 else None, c + pdy2, ptr(B.xb), c + px, ptr(B.mean), ptr(B.invstd),
                             ptr(B.gamma), ptr(B.beta), dx.ptr, c + pdx, ptr(dres), c + pdres, dg.ptr, db.ptr, rows, c, int(rm != 0), training,
                             sums.ptr, ptr(mask_bytes) if rm == 1 else None, None), "s16_bn_bwd")
    sync()
    guards(dx, dres, dg, db, sums, what=f"bn_bwd has2 {has2} rm {rm} training {training} dres {want_dres}")
    return dx, dres, dg, db, sums


@functools.lru_cache(maxsize=2)
def _bwd_refs(fam, rows, c):
    """the float64 references and magnitudes of one shape, taken once and shared by its pad patterns (never modified)"""
    I = R.bn_inputs(fam, rows, c)
    if fam == "gauss":                                          # the batch statistics, as fp32 values
        m, s, _ = R.bn_stats_from_sums(R.colstats_ref(I.x)[0], rows)
        mean, invstd = m.float().double(), s.float().double()
    else:
        mean, invstd = I.mean, I.invstd
    v_plain, mag_plain = R.bn_fwd_ref(I.x, mean, invstd, I.gamma, I.beta)
    unsure = R.unsure_of(v_plain, mag_plain, R.K_V_NORES)       # the sign recomputed from x and beta (bn_val: four roundings)
    pos_plain, pos_res = v_plain > 0, (v_plain + I.res) > 0
    forms = {}
    for has2 in (False, True):
        for rm in (0, 1, 2):
            # mask bytes are an input (any bytes do): the residual-free signs without dy2, the signs with a residual with it
            pos = None if rm == 0 else (pos_plain if rm == 2 or not has2 else pos_res)
            b = R.bn_bwd_ref(I.dy, I.dy2 if has2 else None, I.x, mean, invstd, None if pos is None else pos.double())
            e1 = e2 = None
            if rm == 2:
                e1, e2 = (unsure * b.g0mag).sum(0, keepdim=True), (unsure * b.g0mag * b.xhmag).sum(0, keepdim=True)
            forms[(has2, rm)] = (b, e1, e2) + R.bn_bwd_dx_eval(b, I.gamma, invstd)
    return R.Bag(I=I, mean64=mean, invstd64=invstd, unsure=unsure, sure=~unsure, bytes_plain=R.sign_bytes(pos_plain),
                 bytes_res=R.sign_bytes(pos_res), forms=forms)


def _bwd_setup(fam, rows, c, pads):
    ref = _bwd_refs(fam, rows, c)
    I = ref.I
    pdy, pdy2, px, pdx, pdres = pads
    return R.Bag(ref, rows=rows, c=c, pads=pads, dyb=put16(I.dy, c + pdy), dy2b=put16(I.dy2, c + pdy2), xb=put16(I.x, c + px),
                 mean=vec32(ref.mean64), invstd=vec32(ref.invstd64), gamma=vec32(I.gamma), beta=vec32(I.beta))


SKIPPED_ROUTE_CHECKS = [0, 0]                              # train-mode dx, mask bytes against recomputed signs: [skipped, asserted]


@pytest.mark.parametrize("pads", list(R.BWD_PADS))
@pytest.mark.parametrize("rows,c", R.BN_SHAPES)
@pytest.mark.parametrize("fam", FAMILIES)
def test_bn_bwd_all_reduce_instantiations(L, fam, rows, c, pads):
    lib, check = L
    B = _bwd_setup(fam, rows, c, R.BWD_PADS[pads])
    I, invstd, sure = B.I, B.invstd64, B.sure
    assert R.unsure_share(B.unsure) <= R.UNSURE_CAP            # from the reference alone
    bytes_plain, bytes_res = B.bytes_plain, B.bytes_res
    kb, kg = R.k_dbeta(rows, c), R.k_dgamma(rows, c)
    outs = {}
    for has2 in (False, True):
        for rm in (0, 1, 2):
            b, e1, e2, dxe, dxe_mag = B.forms[(has2, rm)]
            es = sure if rm == 2 else None
            if fam == "int":
                R.assert_exact(b.s1mag, 4 * b.s2mag, 4 * dxe_mag)
            for training in (0, 1):
                for want_dres in (True, False):
                    what = f"{fam} {rows} x {c} {pads} has2 {has2} rm {rm} training {training} dres {want_dres}"
                    dx, dres, dg, db, sums = _bwd_call(lib, check, B, has2, rm, training, want_dres, bytes_plain if not has2 else bytes_res)
                    assert torch.equal(sums.t[0].float(), torch.cat([db.t[0], dg.t[0]])), what + ": sums != (dbeta, dgamma) in double"
                    if fam == "int":
                        exact(db.t[0], b.s1, False, what + " dbeta", "bn_bwd dbeta")
                        exact(dg.t[0], b.s2, False, what + " dgamma", "bn_bwd dgamma")
                        exact(sums.t[0], torch.cat([b.s1, b.s2]), False, what + " sums", "bn_bwd sums")
                        if dres is not None:
                            exact(dres.dense(), b.g, True, what + " dres", "bn_bwd dres", sure=es)
                    else:
                        gate(db.t, b.s1[None], b.s1mag[None], kb, False, what + " dbeta", "bn_bwd dbeta", extra=e1)
                        gate(dg.t, b.s2[None], b.s2mag[None], kg, False, what + " dgamma", "bn_bwd dgamma", extra=e2)
                        if dres is not None:
                            gate(dres.f64(), b.g, b.gmag, R.K_DRES, True, what + " dres", "bn_bwd dres", sure=es)
                    if training:
                        ref, mag = R.bn_bwd_dx_train(b, I.gamma, invstd, db.f64()[0], dg.f64()[0], rows)      # the sums the kernel wrote
                        gate(dx.f64(), ref, mag, R.K_DX_TRAIN, True, what + " dx", "bn_bwd dx train", sure=es)
                    elif fam == "int":
                        exact(dx.dense(), dxe, True, what + " dx", "bn_bwd dx eval", sure=es)
                    else:
                        gate(dx.f64(), dxe, dxe_mag, R.K_DX_EVAL, True, what + " dx", "bn_bwd dx eval", sure=es)
                    outs[(has2, rm, training, want_dres)] = (dx.dense(), None if dres is None else dres.dense(), dg.t[0].clone(), db.t[0].clone())
    # without a residual the mask-byte route and the recompute route agree on sure elements
    for training in (0, 1):
        for want_dres in (True, False):
            a, r = outs[(False, 1, training, want_dres)], outs[(False, 2, training, want_dres)]
            if want_dres:
                assert same_bits(a[1][sure], r[1][sure]), "dres: mask bytes against recomputed signs"
            # train-mode dx goes through dbeta / dgamma: the two routes' sums meet in f64 atomics in no fixed order and differ on
            # unsure elements, so their fp32 values may differ in the last bit; dx is then compared bit for bit only where both
            # routes wrote the same sums (each dx has passed its own interval above either way).  The module prints the count.
            if not training or (torch.equal(a[2], r[2]) and torch.equal(a[3], r[3])):
                assert same_bits(a[0][sure], r[0][sure]), "dx: mask bytes against recomputed signs"
                SKIPPED_ROUTE_CHECKS[1] += int(training)
            else:
                SKIPPED_ROUTE_CHECKS[0] += 1


def test_bn_bwd_and_colstats_at_the_slice_cap(L):
    """8 500 x 4 096: red_geom<8> caps the grid at 1 024 / 32 column blocks = 32 slices of 266 rows (17 rows per thread).  This case
    is about the reduce half: sums, dbeta, dgamma and dres are gated for equality; dx is held under guards (intact, written) and
    deliberately NOT compared here -- the apply half has no path that depends on the slice count, and the shapes above gate it."""
    lib, check = L
    rows, c = R.BIG_SHAPE
    assert R.red_geometry(rows, c)[2:] == (32, 266, 17)
    g = torch.Generator(device=DEV).manual_seed(71)
    ri = lambda lo, hi, shape=(rows, c): torch.randint(lo, hi + 1, shape, generator=g, device=DEV).to(BF)
    xb, dyb, dy2b = ri(-3, 3), ri(-2, 2), ri(-2, 2)
    x, dy, dy2 = xb.double(), dyb.double(), dy2b.double()
    I = R.bn_inputs("int", 5, c)                               # its coefficient vectors
    ref, mag = R.colstats_ref(x)
    R.assert_exact(mag)
    sums = Guarded(2, c, dtype=F64).fill(torch.zeros(2, c))
    check(lib.glf_s16_colstats(ptr(xb), c, rows, c, sums.ptr, None), "s16_colstats")
    sync()
    guards(sums, what="colstats")
    exact(sums.f64(), ref, False, "colstats at the slice cap", "colstats sums")
    v, vmag = R.bn_fwd_ref(x, I.mean, I.invstd, I.gamma, I.beta)
    assert not bool(R.unsure_of(v, vmag, R.K_V_NORES).any())
    b = R.bn_bwd_ref(dy, dy2, x, I.mean, I.invstd, (v > 0).double())
    R.assert_exact(b.s1mag, 4 * b.s2mag)
    B = R.Bag(rows=rows, c=c, pads=(0,) * 5, dyb=dyb, dy2b=dy2b, xb=xb, mean=vec32(I.mean), invstd=vec32(I.invstd), gamma=vec32(I.gamma),
              beta=vec32(I.beta))
    dx, dres, dg, db, bs = _bwd_call(lib, check, B, True, 2, 1, True, None)
    exact(db.t[0], b.s1, False, "dbeta at the slice cap", "bn_bwd dbeta")
    exact(dg.t[0], b.s2, False, "dgamma at the slice cap", "bn_bwd dgamma")
    exact(bs.t[0], torch.cat([b.s1, b.s2]), False, "sums at the slice cap", "bn_bwd sums")
    exact(dres.dense(), b.g, True, "dres at the slice cap", "bn_bwd dres")


# ------------------------------------------------------------------- the same reduce body on fp32 storage (glf_bn_bwd, fused form)
def _bwd_call32(lib, check, dy, dy2, x, V, rows, c, rm, training, want_dres, mask_bytes):
    """glf_bn_bwd in its two-launch form (fused_sums: 2 c doubles of sums, then 2 c floats of maxima) on dense fp32 tensors"""
    dx, dres = Guarded(rows, c), (Guarded(rows, c) if want_dres else None)
    dg, db = Guarded(1, c), Guarded(1, c)
    fs = Guarded(1, 3 * c, dtype=F64).fill(torch.zeros(1, 3 * c))
    check(lib.glf_bn_bwd(ptr(dy), c, ptr(x), c, None, c, ptr(V.mean), ptr(V.invstd), ptr(V.gamma), ptr(V.beta), dx.ptr, c, ptr(dres), c,
                         dg.ptr, db.ptr, rows, c, int(rm != 0), training, None, None, 0, ptr(mask_bytes) if rm == 1 else None, ptr(dy2), c,
                         fs.ptr, None), "bn_bwd")
    sync()
    guards(dx, dres, dg, db, fs, what=f"fp32 bn_bwd has2 {dy2 is not None} rm {rm} training {training} dres {want_dres}")
    assert not bool(fs.t[0, 2 * c:].any()), "the maxima were not asked for"
    return dx, dres, dg, db, fs.t[0, :2 * c]


def test_bn_bwd_fp32_storage_at_the_slice_cap(L):
    """4 100 x 4 096 on fp32 storage: red_geom<4> caps the grid at 1 024 / 64 column blocks = 16 slices of 257 rows -- 17 rows per
    thread, four unrolled trips and a one-row tail -- with the fan-in pair, the sign recomputed from x and dres written by the
    reduce pass.  As at the bf16 cap, this is about the reduce half: sums, dbeta, dgamma and dres are gated for equality."""
    lib, check = L
    rows, c = 4100, 4096
    assert R.red_geometry(rows, c, 4)[2:] == (16, 257, 17)
    g = torch.Generator(device=DEV).manual_seed(72)
    ri = lambda lo, hi: torch.randint(lo, hi + 1, (rows, c), generator=g, device=DEV).to(F32)
    xf, dyf, dy2f = ri(-3, 3), ri(-2, 2), ri(-2, 2)
    x, dy, dy2 = xf.double(), dyf.double(), dy2f.double()
    I = R.bn_inputs("int", 5, c)                               # its coefficient vectors
    v, vmag = R.bn_fwd_ref(x, I.mean, I.invstd, I.gamma, I.beta)
    assert not bool(R.unsure_of(v, vmag, R.K_V_NORES).any())
    b = R.bn_bwd_ref(dy, dy2, x, I.mean, I.invstd, (v > 0).double())
    R.assert_exact(b.s1mag, 4 * b.s2mag)
    V = R.Bag(mean=vec32(I.mean), invstd=vec32(I.invstd), gamma=vec32(I.gamma), beta=vec32(I.beta))
    dx, dres, dg, db, sums = _bwd_call32(lib, check, dyf, dy2f, xf, V, rows, c, 2, 1, True, None)
    exact(db.t[0], b.s1, False, "fp32 dbeta at the slice cap", "bn_bwd fp32 dbeta")
    exact(dg.t[0], b.s2, False, "fp32 dgamma at the slice cap", "bn_bwd fp32 dgamma")
    exact(sums, torch.cat([b.s1, b.s2]), False, "fp32 sums at the slice cap", "bn_bwd fp32 sums")
    exact(dres.dense(), b.g, False, "fp32 dres at the slice cap", "bn_bwd fp32 dres")


@pytest.mark.parametrize("rows,c", [(5, 8), (70, 72), (297, 136), (1031, 264)])
def test_bn_bwd_reduce_is_one_body_for_both_storages(L, rows, c):
    """The integer family (every value exact in bf16, every sum exact in fp32) through glf_bn_bwd's fused form and glf_s16_bn_bwd:
    one reduce body at four and at eight elements per access, mask bytes built at four and at eight signs per byte.  (5, 8): one
    lane per row at eight per access; (70, 72): nine column groups, fewer than a block; (297, 136): a second, ragged column block
    at eight per access, three at four; (1031, 264).  sums, dbeta and dgamma are equal bit for bit across storages, dres after the
    cast -- with and without dres, which on fp32 storage decides whether the reduce pass writes it."""
    lib, check = L
    I = R.bn_inputs("int", rows, c)
    v, vmag = R.bn_fwd_ref(I.x, I.mean, I.invstd, I.gamma, I.beta)
    assert not bool(R.unsure_of(v, vmag, R.K_V_NORES).any())
    pos = {2: v > 0, 1: (v + I.res) > 0}
    V = R.Bag(mean=vec32(I.mean), invstd=vec32(I.invstd), gamma=vec32(I.gamma), beta=vec32(I.beta))
    B = R.Bag(V, rows=rows, c=c, pads=(0,) * 5, dyb=put16(I.dy), dy2b=put16(I.dy2), xb=put16(I.x))
    x32, dy32, dy232 = I.x.float(), I.dy.float(), I.dy2.float()
    for has2 in (False, True):
        for rm in (0, 1, 2):
            b = R.bn_bwd_ref(I.dy, I.dy2 if has2 else None, I.x, I.mean, I.invstd, None if rm == 0 else pos[rm].double())
            R.assert_exact(b.s1mag, 4 * b.s2mag)
            m8, m4 = (R.sign_bytes(pos[1], 8), R.sign_bytes(pos[1], 4)) if rm == 1 else (None, None)
            for want_dres in (True, False):
                what = f"{rows} x {c} has2 {has2} rm {rm} dres {want_dres}"
                _, dres16, dg16, db16, s16 = _bwd_call(lib, check, B, has2, rm, 1, want_dres, m8)
                _, dres32, dg32, db32, s32 = _bwd_call32(lib, check, dy32, dy232 if has2 else None, x32, V, rows, c, rm, 1, want_dres, m4)
                assert torch.equal(s16.t[0], s32) and same_bits(dg16.t[0], dg32.t[0]) and same_bits(db16.t[0], db32.t[0]), what + ": sums across storages"
                exact(s32, torch.cat([b.s1, b.s2]), False, what + " sums", "bn_bwd fp32 sums")
                if want_dres:
                    assert same_bits(dres32.dense().to(BF), dres16.dense()), what + ": dres across storages"
                    exact(dres32.dense(), b.g, False, what + " dres", "bn_bwd fp32 dres")


# -------------------------------------------------------------------------------------------------------------- TPAVI tail
@pytest.mark.parametrize("rows", R.TAIL_ROWS)
@pytest.mark.parametrize("c", R.TAIL_C)
@pytest.mark.parametrize("fam", FAMILIES)
def test_bn_res_ln_tail(L, fam, rows, c):
    lib, check = L
    I = R.tail_inputs(fam, rows, c)
    wb, xb, dzb = put16(I.w), put16(I.x), put16(I.dz)
    V = {k: vec32(I[k]) for k in ("mean", "invstd", "bn_g", "bn_b", "ln_g", "ln_b")}
    what = f"{fam} {rows} x {c}"
    u, umag = R.tail_u(I)
    z, rmu, rrs = Guarded16(rows, c), Guarded(1, rows), Guarded(1, rows)
    check(lib.glf_s16_bn_res_ln_fwd(ptr(wb), ptr(xb), ptr(V["mean"]), ptr(V["invstd"]), ptr(V["bn_g"]), ptr(V["bn_b"]), ptr(V["ln_g"]), ptr(V["ln_b"]),
                                    R.LN_EPS, z.ptr, rmu.ptr, rrs.ptr, rows, c, None), "s16_bn_res_ln_fwd")
    sync()
    guards(z, rmu, rrs, what=what + " fwd")
    gate(rmu.t[0], *R.tail_row_mean(u, umag), R.K_ROW_MEAN, False, what + " row_mean", "tail row_mean")
    m_hat = rmu.f64()[0]
    gate(rrs.t[0], *R.tail_row_rstd(u, umag, m_hat), R.K_ROW_RSTD, False, what + " row_rstd", "tail row_rstd")
    r_hat = rrs.f64()[0]
    gate(z.f64(), *R.tail_z(u, umag, m_hat, r_hat, I.ln_g, I.ln_b), R.K_Z, True, what + " z", "tail z")

    nbytes = int(lib.glf_s16_bn_res_ln_workspace(rows, c))
    assert nbytes == ((rows + R.LN_ROWS - 1) // R.LN_ROWS) * 2 * c * 4
    runs = []
    for _ in range(2):
        du, dg, db, ws = Guarded16(rows, c), Guarded(1, c), Guarded(1, c), Guarded(1, nbytes // 4)
        check(lib.glf_s16_bn_res_ln_bwd(ptr(dzb), ptr(wb), ptr(xb), ptr(V["mean"]), ptr(V["invstd"]), ptr(V["bn_g"]), ptr(V["bn_b"]), ptr(V["ln_g"]),
                                        rmu.ptr, rrs.ptr, du.ptr, dg.ptr, db.ptr, rows, c, ws.ptr, None), "s16_bn_res_ln_bwd")
        sync()
        guards(du, dg, db, ws, what=what + " bwd")
        runs.append((du, dg, db))
    du, dg, db = runs[0]
    b = R.tail_bwd_ref(u, umag, I.dz, m_hat, r_hat, I.ln_g)
    gate(du.f64(), b.du, b.dumag, R.K_DU, True, what + " du", "tail du")
    gate(dg.t[0], b.dg, b.dgmag, R.K_DLN_G, False, what + " dln_gamma", "tail dln_gamma")
    if fam == "int":
        R.assert_exact(b.dbmag)
        exact(db.t[0], b.db, False, what + " dln_beta", "tail dln_beta")
    else:
        gate(db.t[0], b.db, b.dbmag, R.K_DLN_B, False, what + " dln_beta", "tail dln_beta")
    for a, r in zip(runs[0], runs[1]):
        assert torch.equal(a.buf, r.buf), what + ": two runs differ"


# ---------------------------------------------------------------------------------------------------------------- row sums
@pytest.mark.parametrize("c", R.SUM_C)
@pytest.mark.parametrize("p", R.SUM_P)
def test_sum_rows(L, p, c):
    lib, check = L
    inv_p = float(torch.tensor(1.0 / p, dtype=F32))
    for fam, scale in (("int", 0.5), ("gauss", inv_p)):
        for n in R.SUM_N:
            x = R.sum_inputs(fam, n, p, c)
            ref, mag = R.sum_rows_ref(x, n, p, scale)
            if fam == "int":
                R.assert_exact(2 * mag)
            for pad in (0, 8):
                xb = put16(x, c + pad)
                for dt in (DT_F32, DT_BF16):
                    y = Guarded(n, c) if dt == DT_F32 else Guarded16(n, c)
                    check(lib.glf_s16_sum_rows(ptr(xb), c + pad, y.ptr, dt, scale, n, p, c, None), "s16_sum_rows")
                    sync()
                    what = f"{fam} n {n} p {p} c {c} pad {pad} {'fp32' if dt == DT_F32 else 'bf16'}"
                    guards(y, what=what)
                    if fam == "int":
                        exact(y.dense(), ref, dt == DT_BF16, what, "sum_rows y")     # bf16: bf16_rne of the exact fp32 result
                    else:
                        gate(y.f64(), ref, mag, R.k_sum_rows(p), dt == DT_BF16, what, "sum_rows y")


# ------------------------------------------------------------------------------------------------------------------- casts
def _tile(t, n):
    return t.repeat((n + t.numel() - 1) // t.numel())[:n].contiguous()


def test_cast_bit_exact_against_torch(L):
    lib, check = L
    two_passes = torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 * 8 + 8       # the grid-stride loop turns twice
    spec, nans = R.cast_specials(), R.cast_nans()
    ties = spec[((spec & 0xFFFF) == 0x8000)][:8]
    all16 = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16)       # every bf16 bit pattern
    for n, src_bits in ((8, ties), (spec.numel(), spec), (two_passes, _tile(spec, two_passes))):
        src = src_bits.view(F32)
        want = src.to(BF).view(torch.int16)                     # torch on the CPU: round to nearest, ties to even
        dst = Guarded16(1, n)
        check(lib.glf_s16_cast(ptr(src.to(DEV)), DT_F32, dst.ptr, DT_BF16, n, None), "s16_cast f32 -> bf16")
        sync()
        guards(dst, what=f"f32 -> bf16, {n}")
        bad = (dst.t[0].cpu() != want).nonzero()
        assert bad.numel() == 0, f"f32 -> bf16, {n}: first at {int(bad[0])}: {int(src_bits[bad[0]]) & 0xFFFFFFFF:#x} -> {int(dst.t[0][bad[0]]) & 0xFFFF:#x}, want {int(want[bad[0]]) & 0xFFFF:#x}"
    dst = Guarded16(1, 8)
    check(lib.glf_s16_cast(ptr(nans.view(F32).to(DEV)), DT_F32, dst.ptr, DT_BF16, 8, None), "s16_cast(NaN)")
    sync()
    assert dst.intact() and bool(dst.dense().isnan().all()), "NaN must stay NaN"
    for n, src_bits in ((8, all16[32768 + 0x3F80:32768 + 0x3F88].contiguous()), (65536, all16), (two_passes, _tile(all16, two_passes))):
        src = src_bits.view(BF)
        want = src.float()
        dst = Guarded(1, n)
        check(lib.glf_s16_cast(ptr(src.to(DEV)), DT_BF16, dst.ptr, DT_F32, n, None), "s16_cast bf16 -> f32")
        sync()
        guards(dst, what=f"bf16 -> f32, {n}")
        got = dst.t[0].cpu()
        nan = want.isnan()
        assert torch.equal(got.isnan(), nan) and torch.equal(got.view(torch.int32)[~nan], want.view(torch.int32)[~nan]), f"bf16 -> f32, {n}"


# --------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_launch_nothing(L):
    lib, _ = L
    rows, c = 16, 64
    x = put16(torch.zeros(rows + 1, 4104, dtype=F64))           # wide enough for every shape below
    f = torch.ones(4104, dtype=F32, device=DEV)
    out16, outf, outd, outb = Guarded16(rows + 1, 4104), Guarded(3, 4104), Guarded(2, 4104, dtype=F64), Guarded(1, 4104, dtype=torch.uint8)
    everything = (out16, outf, outd, outb)

    def refused(rc, status, fragment):
        msg = lib.glf_last_error().decode()
        assert rc == status and fragment in msg, (rc, status, msg)
        sync()
        assert all(g.untouched() for g in everything), "a refused call wrote: " + fragment

    X, Y, FP, O = ptr(x), out16.ptr, ptr(f), outf.ptr
    apply = lambda x_=X, ldx=c, res=None, ldr=c, y=Y, ldy=c, rows_=rows, c_=c, rmean=None, rvar=None: lib.glf_s16_bn_apply(
        x_, ldx, res, ldr, y, ldy, outd.ptr, rows_, c_, R.EPS, R.MOM, FP, FP, O, O + 4 * 4104, rmean, rvar, None, 1, outb.ptr, None)
    bwd = lambda dy=X, lddy=c, dy2=None, lddy2=c, ldx=c, beta=FP, dx=Y, lddx=c, dres=None, lddres=c, rows_=rows, c_=c, relu=1, mask=None: lib.glf_s16_bn_bwd(
        dy, lddy, dy2, lddy2, X, ldx, FP, FP, FP, beta, dx, lddx, dres, lddres, O, O + 4 * 4104, rows_, c_, relu, 1, outd.ptr, mask, None)
    tail_f = lambda c_=c, rows_=rows, w=X: lib.glf_s16_bn_res_ln_fwd(w, X, FP, FP, FP, FP, FP, FP, R.LN_EPS, Y, O, O + 4 * 4104, rows_, c_, None)
    tail_b = lambda c_=c, rows_=rows, dz=X: lib.glf_s16_bn_res_ln_bwd(dz, X, X, FP, FP, FP, FP, FP, FP, FP, Y, O, O + 4 * 4104, rows_, c_, O + 8 * 4104, None)
    c8, ld8, al = "channel count must be a positive multiple of 8", "must be a multiple of 8", "must be 16-byte aligned"
    # C % 8 != 0
    refused(lib.glf_s16_colstats(X, c, rows, 60, outd.ptr, None), ERR_BAD_SHAPE, c8)
    refused(lib.glf_s16_colsum(X, c, O, rows, 60, outd.ptr, None), ERR_BAD_SHAPE, c8)
    refused(apply(c_=60), ERR_BAD_SHAPE, c8)
    refused(bwd(c_=60), ERR_BAD_SHAPE, c8)
    refused(tail_f(c_=60), ERR_BAD_SHAPE, c8)
    refused(tail_b(c_=60), ERR_BAD_SHAPE, c8)
    refused(lib.glf_s16_sum_rows(X, c, O, DT_F32, 1.0, 1, rows, 60, None), ERR_BAD_SHAPE, c8)
    # a stride % 8 != 0
    refused(lib.glf_s16_colstats(X, c + 4, rows, c, outd.ptr, None), ERR_BAD_SHAPE, "ldx " + ld8)
    refused(lib.glf_s16_colsum(X, c + 4, O, rows, c, outd.ptr, None), ERR_BAD_SHAPE, "lddy " + ld8)
    refused(apply(ldx=c + 4), ERR_BAD_SHAPE, "ldx " + ld8)
    refused(apply(ldy=c + 4), ERR_BAD_SHAPE, "ldy " + ld8)
    refused(apply(res=X, ldr=c + 4), ERR_BAD_SHAPE, "ldr " + ld8)
    refused(bwd(lddy=c + 4), ERR_BAD_SHAPE, "lddy " + ld8)
    refused(bwd(dy2=X, lddy2=c + 4), ERR_BAD_SHAPE, "lddy2 " + ld8)
    refused(bwd(ldx=c + 4), ERR_BAD_SHAPE, "ldx " + ld8)
    refused(bwd(lddx=c + 4), ERR_BAD_SHAPE, "lddx " + ld8)
    refused(bwd(dres=Y, lddres=c + 4), ERR_BAD_SHAPE, "lddres " + ld8)
    refused(lib.glf_s16_sum_rows(X, c + 4, O, DT_F32, 1.0, 1, rows, c, None), ERR_BAD_SHAPE, "ldx " + ld8)
    # a misaligned pointer
    refused(lib.glf_s16_colstats(X + 8, c, rows, c, outd.ptr, None), ERR_BAD_SHAPE, "x " + al)
    refused(lib.glf_s16_colsum(X + 8, c, O, rows, c, outd.ptr, None), ERR_BAD_SHAPE, "dy " + al)
    refused(apply(x_=X + 8), ERR_BAD_SHAPE, "x " + al)
    refused(apply(y=Y + 8), ERR_BAD_SHAPE, "y " + al)
    refused(apply(res=X + 8), ERR_BAD_SHAPE, "residual " + al)
    refused(bwd(dy=X + 8), ERR_BAD_SHAPE, "dy " + al)
    refused(bwd(dx=Y + 8), ERR_BAD_SHAPE, "dx " + al)
    refused(bwd(dres=Y + 8), ERR_BAD_SHAPE, "dres " + al)
    refused(bwd(dy2=X + 8), ERR_BAD_SHAPE, "dy2 " + al)
    refused(tail_f(w=X + 8), ERR_BAD_SHAPE, "w " + al)
    refused(tail_b(dz=X + 8), ERR_BAD_SHAPE, "dz " + al)
    refused(lib.glf_s16_sum_rows(X + 8, c, O, DT_F32, 1.0, 1, rows, c, None), ERR_BAD_SHAPE, "x " + al)
    refused(lib.glf_s16_cast(X + 8, DT_BF16, O, DT_F32, 64, None), ERR_BAD_SHAPE, "src " + al)
    refused(lib.glf_s16_cast(X, DT_BF16, O + 8, DT_F32, 64, None), ERR_BAD_SHAPE, "dst " + al)
    # beyond the channel limits
    refused(apply(c_=4104, ldx=4104, ldy=4104), ERR_UNSUPPORTED, "s16_bn_apply: C must be <= 4096")
    refused(bwd(c_=4104, lddy=4104, ldx=4104, lddx=4104), ERR_UNSUPPORTED, "s16_bn_bwd: C must be <= 4096")
    refused(tail_f(c_=2056), ERR_UNSUPPORTED, "s16_bn_res_ln: C must be <= 2048")
    refused(tail_b(c_=2056), ERR_UNSUPPORTED, "s16_bn_res_ln: C must be <= 2048")
    # rows = 0
    refused(lib.glf_s16_colstats(X, c, 0, c, outd.ptr, None), ERR_BAD_SHAPE, "rows must be > 0")
    refused(lib.glf_s16_colsum(X, c, O, 0, c, outd.ptr, None), ERR_BAD_SHAPE, "rows must be > 0")
    refused(apply(rows_=0), ERR_BAD_SHAPE, "rows must be > 0")
    refused(bwd(rows_=0), ERR_BAD_SHAPE, "rows must be > 0")
    refused(tail_f(rows_=0), ERR_BAD_SHAPE, "rows must be > 0")
    refused(tail_b(rows_=0), ERR_BAD_SHAPE, "rows must be > 0")
    refused(lib.glf_s16_sum_rows(X, c, O, DT_F32, 1.0, 1, 0, c, None), ERR_BAD_SHAPE, "bad extents")
    # relu without beta and mask; running_mean without running_var; casts
    refused(bwd(beta=None, mask=None), ERR_NULL, "needs relu_mask or beta")
    refused(apply(rmean=O + 8 * 4104), ERR_NULL, "both be set or both NULL")
    refused(apply(rvar=O + 8 * 4104), ERR_NULL, "both be set or both NULL")
    refused(lib.glf_s16_cast(X, DT_BF16, Y, DT_BF16, 64, None), ERR_UNSUPPORTED, "built for bf16 -> f32 and f32 -> bf16")
    refused(lib.glf_s16_cast(FP, DT_F32, O, DT_F32, 64, None), ERR_UNSUPPORTED, "built for bf16 -> f32 and f32 -> bf16")
    refused(lib.glf_s16_cast(X, DT_BF16, O, DT_F32, 60, None), ERR_BAD_SHAPE, "positive multiple of 8")
    refused(lib.glf_s16_cast(X, DT_BF16, O, DT_F32, 0, None), ERR_BAD_SHAPE, "positive multiple of 8")
    refused(lib.glf_s16_sum_rows(X, c, O, 7, 1.0, 1, rows, c, None), ERR_UNSUPPORTED, "y_dtype must be")
