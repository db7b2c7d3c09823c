"""GPU: the column-owning BatchNorm streaming passes (glf_bn_apply, glf_bn_apply_from_sums, glf_bn_bwd) at the shapes where the
thread mapping can go wrong -- fewer rows than a workgroup has row lanes, row counts that run the four-row main loop and the
tail loop, fewer float4 lanes than a column block, exactly one block, a partial second block, the in-kernel-statistics limit
and the route past it, row strides larger than C -- against float64, with sentinel guards around every output buffer.

Tolerances (|err| <= tol + tol |ref|) are those of tests/test_gpu_ops.py: y 2e-5, dx 1e-4, dgamma / dbeta 2e-4, dres 1e-5,
running_mean 1e-6, running_var 1e-5 (test_batch_norm_act); mean / invstd 1e-6 (a float64 result rounded once to fp32 is within
6e-8 relative); a packed image reconstructs to 2^-21 of its bound (+ 2e-6 of it between two runs of the two-launch form, whose
f64 atomics meet in no fixed order), and the forward bound is within 4x of the true maximum."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, MOM = 1e-5, 0.1
SENT_F, SENT_B, GUARD = -1234.5, 0xA5, 64

ROWS = [5, 70, 297, 1031]
CHANNELS = [4, 8, 64, 72, 2048, 4096, 4100]          # 4100: past the in-kernel-statistics limit (the other route)


def _p(t):
    return None if t is None else t.data_ptr()


def rnd(*shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV)


class Guarded:
    """[rows][ld] output whose first c columns the kernel may write: everything else (GUARD elements before and after, the
    columns c .. ld of every row) holds a sentinel that must survive."""

    def __init__(self, rows, c, ld=None, dtype=torch.float32):
        ld = c if ld is None else ld
        self.sent = SENT_B if dtype == torch.uint8 else SENT_F
        self.buf = torch.full((GUARD + rows * ld + GUARD,), self.sent, dtype=dtype, device=DEV)
        self.body = self.buf[GUARD:GUARD + rows * ld].view(rows, ld)
        self.t = self.body[:, :c]
        self.ld, self.c = ld, c

    @property
    def ptr(self):
        return self.body.data_ptr()

    def dense(self):
        return self.t.contiguous()

    def intact(self):
        ok = bool((self.buf[:GUARD] == self.sent).all()) and bool((self.buf[-GUARD:] == self.sent).all())
        return ok and (self.ld == self.c or bool((self.body[:, self.c:] == self.sent).all()))

    def written(self):
        return bool((self.t != self.sent).all())


def close(a, b, tol):
    a, b = a.double(), b.double()
    err = (a - b).abs()
    ok = bool((err <= tol + tol * b.abs()).all())
    if not ok:
        print("max abs err", float(err.max()), "max |ref|", float(b.abs().max()), "tol", tol)
    return ok


def unpack(pk, rows, c, bound):
    """fp32 values of a packed pre-split image under the library's scale: the power of two that brings the bound into [2^13, 2^14)"""
    s = 2.0 ** (13 - int(np.floor(np.log2(bound))))
    halves = pk.contiguous().view(torch.float16).view(rows, c // 4, 8).double()
    return ((halves[..., :4] + halves[..., 4:] * 2.0 ** -11) / s).reshape(rows, c)


def sign_bytes(positive):
    rows, c = positive.shape
    b = positive.reshape(rows, c // 4, 4).to(torch.uint8)
    return (b[..., 0] | (b[..., 1] << 1) | (b[..., 2] << 2) | (b[..., 3] << 3)).contiguous()


def make_x(rows, c, ld, seed):
    """x = +-z + 0.3 with |z| in [1, 2], rows paired (z, -z): every channel has mean 0.3, max |x - mean| >= 1 and a standard
    deviation >= ~1, so the forward's a-priori bound |gamma| invstd (max|x| + |mean|) + |beta| is within (max|z| + 0.6) / max|z|
    <= 1.6 of the true maximum for beta >= 0 BY CONSTRUCTION (the 4x check below tests the kernel, not the luck of a seed)."""
    h = rows // 2
    z = rnd(h, c, seed=seed, lo=1.0, hi=2.0) * torch.where(rnd(h, c, seed=seed + 1) > 0, 1.0, -1.0)
    x = torch.cat([z, -z] + ([torch.zeros(1, c, device=DEV)] if rows % 2 else []), 0) + 0.3
    buf = rnd(rows, ld, seed=seed + 2)
    buf[:, :c] = x
    return buf


@pytest.fixture(scope="module")
def lib_f16x3():
    from glfusion_amd import ops as _ops
    from glfusion_amd._lib import lib, check
    _ops.set_precision("f16x3")
    yield lib, check
    _ops.set_precision("f32")


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("rows", ROWS)
def test_bn_forward_both_kernels(lib_f16x3, rows, c, pad):
    lib, check = lib_f16x3
    ld = c + pad
    xb = make_x(rows, c, ld, seed=11)
    x = xb[:, :c]
    rb = rnd(rows, ld, seed=14)
    gamma, beta = rnd(c, seed=15, lo=0.5, hi=1.5), rnd(c, seed=16, lo=0.0, hi=1.0)
    xd = x.double()
    m64, var64 = xd.mean(0), xd.var(0, unbiased=False)
    mean32, is32 = m64.float(), (1.0 / (var64 + EPS).sqrt()).float()
    sums = torch.stack([xd.sum(0), (xd * xd).sum(0)]).contiguous()
    rm0, rv0 = rnd(c, seed=17) * 0.1, rnd(c, seed=18, lo=0.5, hi=1.5)
    unb = var64 * rows / (rows - 1)
    base = (xd - mean32.double()) * is32.double() * gamma.double() + beta.double()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    calls = 0
    for res, relu, want_mask in ((False, False, False), (False, True, False), (True, True, True), (True, False, False), (False, True, True)):
        v = base + rb[:, :c].double() if res else base
        ref = torch.relu(v) if relu else v
        for kernel in ("apply", "sums"):
            if kernel == "sums" and c > 4096:
                assert lib.glf_bn_apply_from_sums(_p(xb), ld, None, ld, _p(xb), ld, _p(sums), rows, c, EPS, MOM, _p(gamma), _p(beta), _p(mean32),
                                                  _p(is32), None, None, None, 0, None, None, None, None) != 0
                continue
            outs = {}
            for inplace in (False, True):
                y = Guarded(rows, c, ld)
                mask = Guarded(1, rows * (c // 4), dtype=torch.uint8) if want_mask else None
                am = torch.zeros(1, device=DEV)
                if inplace:
                    y.t.copy_(x)
                xp = y.ptr if inplace else _p(xb)
                if kernel == "apply":
                    check(lib.glf_bn_apply(xp, ld, _p(rb) if res else None, ld, y.ptr, ld, _p(mean32), _p(is32), _p(gamma), _p(beta), rows, c,
                                           int(relu), _p(am), mask.ptr if mask else None, None), "bn_apply")
                else:
                    mo, io, rm, rv = Guarded(1, c), Guarded(1, c), Guarded(1, c), Guarded(1, c)
                    rm.t.copy_(rm0); rv.t.copy_(rv0)
                    check(lib.glf_bn_apply_from_sums(xp, ld, _p(rb) if res else None, ld, y.ptr, ld, _p(sums), rows, c, EPS, MOM, _p(gamma), _p(beta),
                                                     mo.ptr, io.ptr, rm.ptr, rv.ptr, _p(nbt), int(relu), _p(am), mask.ptr if mask else None, None, None),
                          "bn_apply_from_sums")
                    calls += 1
                    torch.cuda.synchronize()
                    assert int(nbt) == calls, "num_batches_tracked must advance by exactly one per call"
                    for g_ in (mo, io, rm, rv):
                        assert g_.intact() and g_.written()
                    assert close(mo.t[0], m64, 1e-6) and close(io.t[0], 1.0 / (var64 + EPS).sqrt(), 1e-6)
                    assert close(rm.t[0], 0.9 * rm0.double() + 0.1 * m64, 1e-6)
                    assert close(rv.t[0], 0.9 * rv0.double() + 0.1 * unb, 1e-5)
                torch.cuda.synchronize()
                assert y.intact() and y.written(), (kernel, res, relu, inplace)
                assert close(y.t, ref, 2e-5), (kernel, res, relu, inplace)
                assert abs(float(am) - float(y.t.abs().max())) <= 1e-6 * float(y.t.abs().max())
                if mask:
                    assert mask.intact()
                    got = mask.t.view(rows, c // 4)
                    if not res or relu:      # (res without ReLU: y is not rewritten, but its sign is still that of the value stored)
                        assert torch.equal(got, sign_bytes(y.t > 0)), "sign bytes disagree with the y written"
                    sure = (v.abs() > 1e-4)
                    assert torch.equal(sign_bytes((v > 0) & sure), got & sign_bytes(sure)), "sign bytes disagree with float64"
                outs[inplace] = (y.dense(), None if mask is None else mask.dense())
            assert torch.equal(outs[False][0].view(torch.int32), outs[True][0].view(torch.int32)), "in place differs from out of place"
            if want_mask:
                assert torch.equal(outs[False][1], outs[True][1])
            if kernel == "sums" and not res:
                # the packed image (colmax): scaled by a bound known before y is
                colmax = x.abs().amax(0).contiguous()
                pk, bslot = Guarded(rows, c, ld), torch.zeros(1, device=DEV)
                mo, io = Guarded(1, c), Guarded(1, c)
                check(lib.glf_bn_apply_from_sums(_p(xb), ld, None, ld, pk.ptr, ld, _p(sums), rows, c, EPS, MOM, _p(gamma), _p(beta), mo.ptr, io.ptr,
                                                 None, None, _p(nbt), int(relu), _p(bslot), None, _p(colmax), None), "bn_apply_from_sums(colmax)")
                calls += 1
                torch.cuda.synchronize()
                assert int(nbt) == calls
                assert pk.intact() and mo.intact() and io.intact()
                bound, true_max = float(bslot), float(ref.abs().max())
                assert true_max <= bound <= 4.0 * true_max, (true_max, bound)
                err = float((unpack(pk.t, rows, c, bound) - outs[False][0].double()).abs().max())
                assert err <= 2.0 ** -21 * bound, (err, bound)


# ----------------------------------------------------------------------------------------------------------------- backward
def _bwd(lib, check, dy, dy2, xb, ld, ysrc, maskb, mean, invstd, gamma, beta, rows, c, relu, training, packed, ws, fused, want_dres=True):
    dx, dres = Guarded(rows, c, ld), (Guarded(rows, c, ld) if want_dres else None)
    dg, db = Guarded(1, c), Guarded(1, c)
    am = torch.zeros(1, device=DEV)
    fs = torch.zeros(3 * c, dtype=torch.float64, device=DEV) if fused else None
    check(lib.glf_bn_bwd(_p(dy), ld, _p(xb), ld, _p(ysrc), ld, _p(mean), _p(invstd), _p(gamma), _p(beta), dx.ptr, ld,
                         dres.ptr if dres else None, ld, dg.ptr, db.ptr, rows, c, int(relu), int(training), _p(ws), _p(am), packed,
                         _p(maskb), _p(dy2), ld, _p(fs), None), "bn_bwd")
    torch.cuda.synchronize()
    for g_ in (dx, dg, db) + ((dres,) if dres else ()):
        assert g_.intact() and g_.written(), "an output buffer's guard was written, or an element was not"
    return dx.dense(), (dres.dense() if dres else None), dg.t[0].clone(), db.t[0].clone(), float(am)


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("c", CHANNELS)
@pytest.mark.parametrize("rows", ROWS)
def test_bn_backward_all_forms(lib_f16x3, rows, c, pad):
    lib, check = lib_f16x3
    ld = c + pad
    xb = make_x(rows, c, ld, seed=21)
    x = xb[:, :c]
    ab, bb, rb = rnd(rows, ld, seed=24) * 3.0, rnd(rows, ld, seed=25) * 0.7, rnd(rows, ld, seed=26)
    gamma, beta = rnd(c, seed=27, lo=0.5, hi=1.5), rnd(c, seed=28)
    xd = x.double()
    mean, invstd = xd.mean(0).float(), (1.0 / (xd.var(0, unbiased=False) + EPS).sqrt()).float()
    xh = (xd - mean.double()) * invstd.double()
    v_plain = xh * gamma.double() + beta.double()
    v_res = v_plain + rb[:, :c].double()
    # no gradient where a ReLU input is within 1e-3 of zero: the sign the kernel recomputes in fp32 is then the float64 sign
    kink = (v_plain.abs() < 1e-3) | (v_res.abs() < 1e-3)
    ab[:, :c][kink] = 0.0
    bb[:, :c][kink] = 0.0
    sb = (ab + bb).contiguous()                       # the pre-added tensor (the kernels add in fp32, in this order)
    yb = torch.zeros(rows, ld, device=DEV)
    yb[:, :c] = torch.relu(v_res).float()
    maskb = sign_bytes(v_res > 0)
    ws = torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=torch.float64, device=DEV)
    k = (gamma * invstd).double()
    # rm: 0 no ReLU, 1 sign bytes, 2 recomputed from x (no residual), 3 from the saved output y
    for rm in (0, 1, 2, 3):
        relu = rm != 0
        M = torch.ones_like(v_res, dtype=torch.bool) if rm == 0 else ((v_plain > 0) if rm == 2 else (v_res > 0))
        ysrc, mb = (yb if rm == 3 else None), (maskb if rm == 1 else None)
        g = sb[:, :c].double() * M
        s1, s2 = g.sum(0), (g * xh).sum(0)
        for training in (1, 0):
            ref_dx = k * (g - (s1 + xh * s2) / rows) if training else g * k
            fp32 = None
            for packed in (0, 1):
                got = {}
                for has2 in (False, True):
                    for fused in (False, True):
                        dy, dy2 = (ab, bb) if has2 else (sb, None)
                        out = _bwd(lib, check, dy, dy2, xb, ld, ysrc, mb, mean, invstd, gamma, beta, rows, c, relu, training, packed, ws, fused)
                        got[(has2, fused)] = out
                        dx, dres, dg, db, am = out
                        tag = (rm, training, packed, has2, fused)
                        assert close(dres, g, 1e-5), tag
                        assert close(dg, s2, 2e-4) and close(db, s1, 2e-4), tag
                        if not packed:
                            assert close(dx, ref_dx, 1e-4), tag
                            assert abs(am - float(dx.abs().max())) <= 1e-6 * float(dx.abs().max()), tag
                # the pre-added tensor through the three-launch form is the yardstick of the bitwise checks
                dx3, dres3, dg3, db3, am3 = got[(False, False)]
                for key, (dx, dres, dg, db, am) in got.items():
                    assert torch.equal(dres.view(torch.int32), dres3.view(torch.int32)), ("dres", rm, training, packed, key)
                    if not key[1] or c > 4096:      # three launches: no atomics, bit for bit whatever the addends' form
                        assert torch.equal(dx.view(torch.int32), dx3.view(torch.int32)) and torch.equal(dg, dg3) and torch.equal(db, db3) and am == am3
                if packed:
                    for key, (pk, _, _, _, bound) in got.items():
                        true_max = float(fp32[key][0].abs().max())
                        assert true_max <= bound, (true_max, bound)
                        if rows >= 70 or not training:
                            # bound = |k| (max|g| + (|s1| + max|xhat| |s2|) / n): the correction term is O(n^-1/2) of max|g| from 70 rows
                            # on, so the bound stays within 4x as test_bn_backward_writes_packed_gradient asks (at 5 rows the triangle
                            # inequality behind it may cost up to 1 + 1 + max|xhat|^2 = 6x: a property of the data, not of the kernel)
                            assert bound <= 4.0 * true_max, (true_max, bound)
                        err = float((unpack(pk, rows, c, bound) - fp32[key][0].double()).abs().max())
                        assert err <= (2.0 ** -21 + (2e-6 if key[1] else 0.0)) * bound, (err, bound, key)
                else:
                    fp32 = got
                    # the bound of the packed form (bnbwd_finalize's expression), in float64
                    mg, mx = g.abs().amax(0), xh.abs().amax(0)
                    bound = float((k.abs() * (mg + (s1.abs() + mx * s2.abs()) / rows if training else mg)).max())
                    for has2 in (False, True):          # two launches against three: the fused allowance
                        d = float((got[(has2, True)][0].double() - got[(has2, False)][0].double()).abs().max())
                        assert d <= 2e-6 * bound, (d, bound)
            # reproducibility: three launches twice (everything), two launches with the pair twice (dres)
            a1 = _bwd(lib, check, ab, bb, xb, ld, ysrc, mb, mean, invstd, gamma, beta, rows, c, relu, training, 0, ws, False)
            a2 = _bwd(lib, check, ab, bb, xb, ld, ysrc, mb, mean, invstd, gamma, beta, rows, c, relu, training, 0, ws, False)
            assert all(torch.equal(u, w) for u, w in zip(a1[:4], a2[:4])) and a1[4] == a2[4]
            b1 = _bwd(lib, check, ab, bb, xb, ld, ysrc, mb, mean, invstd, gamma, beta, rows, c, relu, training, 1, ws, True)
            b2 = _bwd(lib, check, ab, bb, xb, ld, ysrc, mb, mean, invstd, gamma, beta, rows, c, relu, training, 1, ws, True)
            assert torch.equal(b1[1].view(torch.int32), b2[1].view(torch.int32))


def test_bn_backward_refuses_dres_aliasing_an_input_of_the_pair_form(lib_f16x3):
    """two launches with dy2 and dres: the reduction pass writes dres while dy, dy2 and x are still being read"""
    lib, check = lib_f16x3
    rows, c = 70, 64
    x, a, b = rnd(rows, c, seed=31), rnd(rows, c, seed=32), rnd(rows, c, seed=33)
    mean, invstd, gamma, beta = rnd(c, seed=34), rnd(c, seed=35, lo=0.5, hi=1.5), rnd(c, seed=36, lo=0.5, hi=1.5), rnd(c, seed=37)
    dx, dg, db, am = torch.empty_like(x), torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.zeros(1, device=DEV)
    for alias in (a, b, x):
        fs = torch.zeros(3 * c, dtype=torch.float64, device=DEV)
        assert lib.glf_bn_bwd(_p(a), c, _p(x), c, None, c, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(dx), c, _p(alias), c, _p(dg), _p(db),
                              rows, c, 1, 1, None, _p(am), 0, None, _p(b), c, _p(fs), None) != 0
    torch.cuda.synchronize()


def test_bn_backward_phase_form_shares_one_scale(lib_f16x3):
    """packed_dx = 2 then 3 for two layers whose images are column slices of one buffer under ONE bound, against the same layers
    done with packed_dx = 1 into images of their own: the shared bound is the larger of the two, and both forms reconstruct
    the same dx (each to 2^-21 of the bound its image is scaled with)."""
    lib, check = lib_f16x3
    rows, c, k = 297, 64, 2
    ld = k * c
    G = Guarded(rows, ld)
    shared = torch.zeros(1, device=DEV)
    ws = torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=torch.float64, device=DEV)
    layers, own = [], []
    for i in range(k):
        xb = make_x(rows, c, c, seed=41 + 10 * i)
        dy = rnd(rows, c, seed=44 + 10 * i) * (3.0 if i == 0 else 0.5)
        gamma, beta = rnd(c, seed=45 + 10 * i, lo=0.5, hi=1.5), rnd(c, seed=46 + 10 * i)
        mean, invstd = xb.double().mean(0).float(), (1.0 / (xb.double().var(0, unbiased=False) + EPS).sqrt()).float()
        keep = torch.empty(2 * c, device=DEV)
        layers.append((xb, dy, gamma, beta, mean, invstd, keep))
        pk, dg, db, am = torch.empty(rows, c, device=DEV), torch.empty(c, device=DEV), torch.empty(c, device=DEV), torch.zeros(1, device=DEV)
        check(lib.glf_bn_bwd(_p(dy), c, _p(xb), c, None, c, _p(mean), _p(invstd), _p(gamma), _p(beta), _p(pk), c, None, c, _p(dg), _p(db),
                             rows, c, 1, 1, _p(ws), _p(am), 1, None, None, 0, None, None), "bn_bwd(1)")
        torch.cuda.synchronize()
        own.append((pk, dg, db, float(am)))
    grads = []
    for i, (xb, dy, gamma, beta, mean, invstd, keep) in enumerate(layers):
        dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        check(lib.glf_bn_bwd(_p(dy), c, _p(xb), c, None, c, _p(mean), _p(invstd), _p(gamma), _p(beta), G.ptr + 4 * i * c, ld, None, c, _p(dg), _p(db),
                             rows, c, 1, 1, _p(ws), _p(shared), 2, None, None, 0, _p(keep), None), "bn_bwd(2)")
        grads.append((dg, db))
    torch.cuda.synchronize()
    assert bool((G.buf == SENT_F).all()), "half 2 must not write the image"
    for i, (xb, dy, gamma, beta, mean, invstd, keep) in enumerate(layers):
        check(lib.glf_bn_bwd(_p(dy), c, _p(xb), c, None, c, _p(mean), _p(invstd), _p(gamma), _p(beta), G.ptr + 4 * i * c, ld, None, c, None, None,
                             rows, c, 1, 1, _p(ws), _p(shared), 3, None, None, 0, _p(keep), None), "bn_bwd(3)")
    torch.cuda.synchronize()
    assert G.intact() and G.written()
    bound = float(shared)
    assert bound == max(o[3] for o in own)
    for i in range(k):
        pk, dg, db, b_own = own[i]
        assert torch.equal(dg, grads[i][0]) and torch.equal(db, grads[i][1])
        a = unpack(G.t[:, i * c:(i + 1) * c], rows, c, bound)
        b = unpack(pk, rows, c, b_own)
        assert float((a - b).abs().max()) <= 2.0 ** -21 * (bound + b_own)
