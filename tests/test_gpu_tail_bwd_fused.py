"""glf_bn_res_ln_bwd_sums: the fusion block's tail backward in ONE walk over dz / w / x -- du, the LayerNorm parameter gradients,
the BatchNorm-backward sums of w and the bound of the packed dwz image -- followed by the apply half of glf_bn_bwd (packed_dx 3 / 4),
against the sequence it replaces (glf_bn_res_ln_bwd, then glf_bn_bwd in its two-launch form) and against float64 on the CPU.

Yardstick for every sum and for dwz (the one test_gpu_aspp_centre.py uses): relative L2 error against float64 computed from the same
fp32 inputs (the saved LayerNorm row statistics included) <= 1.5 x the replaced sequence's error + 1e-7.  Both errors are printed.
du is compared bit for bit.  Shapes: 1 row, fewer rows than a workgroup has waves, more than one batch of rows with a ragged last
one, several slices with ragged slabs (1031) x one live lane, two, a partial wave, the full width."""
import numpy as np
import pytest
import torch

from glfusion_amd._lib import lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROWS = (1, 5, 70, 1031)
CS = (4, 8, 72, 2048)
SENT = -12345.5
GUARD = 64


def _guarded(n, dtype=torch.float32):
    full = torch.full((n + GUARD,), SENT, dtype=dtype, device=DEV)
    return full, full[:n]


def _intact(full, n):
    return bool((full[n:] == SENT).all())


def _rel(a, ref):
    return float((a.detach().cpu().double().reshape(-1) - ref.reshape(-1)).norm()) / max(float(ref.norm()), 1e-300)


def _ws(rows, c):
    return torch.empty(int(lib.glf_bn_workspace(rows, c)), dtype=torch.float64, device=DEV)


def _unpack(img, amax, rows, c):
    """The packed pre-split image {h0..h3 | l0..l3} -> float64 values: x s = h + 2^-11 l, s = 2^(140 - e) for the biased exponent e
    of amax in [20, 250], else 1."""
    e = (int(np.float32(amax).view(np.uint32)) >> 23) & 0xff
    s = 2.0 ** (140 - e) if 20 <= e <= 250 else 1.0
    h = img.detach().cpu().view(torch.float16).view(rows, c // 4, 8).double()
    return ((h[..., :4] + h[..., 4:] / 2048.0) / s).reshape(rows, c)


_INPUTS = {}


def _inputs(rows, c):
    """fp32 inputs on the device, the row statistics the forward saves, and the float64 results; once per shape."""
    key = (rows, c)
    if key in _INPUTS:
        return _INPUTS[key]
    g = torch.Generator().manual_seed(1000 * rows + c)
    t = {
        "dz": torch.randn(rows, c, generator=g), "w": torch.randn(rows, c, generator=g) * 1.7 + 0.3, "x": torch.randn(rows, c, generator=g),
        "mean": torch.randn(c, generator=g) * 0.4, "invstd": torch.rand(c, generator=g) * 1.5 + 0.25,
        "gamma": torch.randn(c, generator=g) * 0.8 + 1.0, "beta": torch.randn(c, generator=g) * 0.3,
        "ln_g": torch.randn(c, generator=g) * 0.5 + 1.0, "ln_b": torch.randn(c, generator=g) * 0.2,
    }
    d = {k: v.to(DEV).contiguous() for k, v in t.items()}
    z = torch.empty(rows, c, device=DEV)
    d["rmu"], d["rrs"] = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    assert lib.glf_bn_res_ln_fwd(d["w"].data_ptr(), d["x"].data_ptr(), d["mean"].data_ptr(), d["invstd"].data_ptr(), d["gamma"].data_ptr(),
                                 d["beta"].data_ptr(), d["ln_g"].data_ptr(), d["ln_b"].data_ptr(), 1e-5, z.data_ptr(), d["rmu"].data_ptr(),
                                 d["rrs"].data_ptr(), rows, c, None, None) == 0
    torch.cuda.synchronize()
    f = {k: v.double() for k, v in t.items()}
    rmu, rrs = d["rmu"].cpu().double()[:, None], d["rrs"].cpu().double()[:, None]
    wh = (f["w"] - f["mean"]) * f["invstd"]
    uh = (wh * f["gamma"] + f["beta"] + f["x"] - rmu) * rrs
    gz = f["dz"] * f["ln_g"]
    du = rrs * (gz - gz.mean(1, keepdim=True) - uh * (gz * uh).mean(1, keepdim=True))
    ref = {"du": du, "dln_g": (f["dz"] * uh).sum(0), "dln_b": f["dz"].sum(0), "dbn_b": du.sum(0), "dbn_g": (du * wh).sum(0)}
    k = f["gamma"] * f["invstd"]
    ref["dwz1"] = k * (du - (ref["dbn_b"] + wh * ref["dbn_g"]) / rows)
    ref["dwz0"] = k * du
    ref["max_wh"] = float(wh.abs().max())
    _INPUTS[key] = (d, ref)
    return _INPUTS[key]


def _fused(rows, c, training, packed):
    """Pass A + the apply half.  -> outputs, guards intact?"""
    d, _ = _inputs(rows, c)
    bufs = {k: _guarded(n) for k, n in (("du", rows * c), ("dln_g", c), ("dln_b", c), ("dbn_g", c), ("dbn_b", c), ("keep", 2 * c),
                                        ("dwz", rows * c))}
    amf = torch.zeros(1 + GUARD, device=DEV)
    amf[1:] = SENT
    ws = _ws(rows, c)
    p = {k: v[1].data_ptr() for k, v in bufs.items()}
    rc = lib.glf_bn_res_ln_bwd_sums(d["dz"].data_ptr(), d["w"].data_ptr(), d["x"].data_ptr(), d["mean"].data_ptr(), d["invstd"].data_ptr(),
                                    d["gamma"].data_ptr(), d["beta"].data_ptr(), d["ln_g"].data_ptr(), d["rmu"].data_ptr(), d["rrs"].data_ptr(),
                                    p["du"], p["dln_g"], p["dln_b"], p["dbn_g"], p["dbn_b"], p["keep"], amf.data_ptr() if packed else None,
                                    rows, c, training, ws.data_ptr(), None)
    assert rc == 0, lib.glf_last_error()
    rc = lib.glf_bn_bwd(p["du"], c, d["w"].data_ptr(), c, None, c, d["mean"].data_ptr(), d["invstd"].data_ptr(), d["gamma"].data_ptr(), None,
                        p["dwz"], c, None, c, None, None, rows, c, 0, training, ws.data_ptr(), amf.data_ptr(), 3 if packed else 4, None, None, 0,
                        p["keep"], None)
    assert rc == 0, lib.glf_last_error()
    torch.cuda.synchronize()
    intact = all(_intact(full, view.numel()) for full, view in bufs.values()) and _intact(amf, 1)
    out = {k: v[1].clone() for k, v in bufs.items()}
    out["amax"] = float(amf[0])
    return out, intact


def _parent(rows, c, training, packed):
    """The replaced sequence: glf_bn_res_ln_bwd, then glf_bn_bwd in its two-launch form on a zeroed slot."""
    d, _ = _inputs(rows, c)
    o = {k: torch.empty(n, device=DEV) for k, n in (("du", rows * c), ("dln_g", c), ("dln_b", c), ("dbn_g", c), ("dbn_b", c), ("dwz", rows * c))}
    am = torch.zeros(1, device=DEV)
    slot = torch.zeros(3 * c + 2, dtype=torch.float64, device=DEV)
    assert lib.glf_bn_res_ln_bwd(d["dz"].data_ptr(), d["w"].data_ptr(), d["x"].data_ptr(), d["mean"].data_ptr(), d["invstd"].data_ptr(),
                                 d["gamma"].data_ptr(), d["beta"].data_ptr(), d["ln_g"].data_ptr(), d["rmu"].data_ptr(), d["rrs"].data_ptr(),
                                 o["du"].data_ptr(), o["dln_g"].data_ptr(), o["dln_b"].data_ptr(), rows, c, _ws(rows, c).data_ptr(), None) == 0
    assert lib.glf_bn_bwd(o["du"].data_ptr(), c, d["w"].data_ptr(), c, None, c, d["mean"].data_ptr(), d["invstd"].data_ptr(), d["gamma"].data_ptr(),
                          None, o["dwz"].data_ptr(), c, None, c, o["dbn_g"].data_ptr(), o["dbn_b"].data_ptr(), rows, c, 0, training, None,
                          am.data_ptr(), int(packed), None, None, 0, slot.data_ptr(), None) == 0
    torch.cuda.synchronize()
    o["amax"] = float(am)
    return o


def _three_launch_bound(rows, c, training, du):
    """glf_bn_bwd packed_dx = 2 (reduction + finalize) on the same du: the bound the packed three-launch form raises."""
    d, _ = _inputs(rows, c)
    am = torch.zeros(1, device=DEV)
    keep, dg, db = torch.empty(2 * c, device=DEV), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx = torch.empty(rows * c, device=DEV)
    assert lib.glf_bn_bwd(du.data_ptr(), c, d["w"].data_ptr(), c, None, c, d["mean"].data_ptr(), d["invstd"].data_ptr(), d["gamma"].data_ptr(), None,
                          dx.data_ptr(), c, None, c, dg.data_ptr(), db.data_ptr(), rows, c, 0, training, _ws(rows, c).data_ptr(), am.data_ptr(), 2,
                          None, None, 0, keep.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return float(am)


_RUNS = {}


def _runs(rows, c, training):
    key = (rows, c, training)
    if key not in _RUNS:
        _RUNS[key] = (_fused(rows, c, training, True), _parent(rows, c, training, True))
    return _RUNS[key]


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_du_bits_sums_and_guards(rows, c):
    (new, intact), old = _runs(rows, c, 1)
    _, ref = _inputs(rows, c)
    assert intact, "a write landed behind an output buffer"
    assert torch.equal(new["du"].view(torch.int32), old["du"].view(torch.int32)), "du differs from glf_bn_res_ln_bwd's"
    assert torch.equal(new["keep"][:c], new["dbn_b"]) and torch.equal(new["keep"][c:], new["dbn_g"])
    for k in ("dln_g", "dln_b", "dbn_g", "dbn_b"):
        e_new, e_old = _rel(new[k], ref[k]), _rel(old[k], ref[k])
        print(f"rows {rows} c {c} {k}: one walk {e_new:.3e} replaced sequence {e_old:.3e}")
        assert e_new <= 1.5 * e_old + 1e-7, (k, e_new, e_old)


@pytest.mark.parametrize("training", [1, 0])
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_bound_and_packed_dwz(rows, c, training):
    (new, intact), old = _runs(rows, c, training)
    _, ref = _inputs(rows, c)
    assert intact
    want = ref["dwz1" if training else "dwz0"]
    true_max = float(want.abs().max())
    assert new["amax"] >= true_max, (new["amax"], true_max)
    # the three-launch form on the same du: max |du| and max |what| are the same bits, the two sums are rounded differently.  Each
    # form sums fp32 over at most 64 rows before going to double: |delta s| <= 64 2^-24 n max|du|, |delta q| that times max|what|,
    # so the bounds k (mg + (|s| + mx |q|) / n) differ by at most 2 x 64 2^-24 (1 + mx^2) relatively; in eval mode not at all
    b3 = _three_launch_bound(rows, c, training, new["du"])
    ratio = new["amax"] / b3
    print(f"rows {rows} c {c} training {training}: bound {new['amax']:.6e} three-launch {b3:.6e} ratio {ratio:.9f} true max {true_max:.6e}")
    tol = 2 * 64 * 2.0 ** -24 * (1 + ref["max_wh"] ** 2) if training else 0.0
    assert abs(ratio - 1.0) <= tol, (ratio, tol)
    e_new = _rel(_unpack(new["dwz"], new["amax"], rows, c), want)
    e_old = _rel(_unpack(old["dwz"], old["amax"], rows, c), want)
    print(f"rows {rows} c {c} training {training} packed dwz: one walk {e_new:.3e} replaced sequence {e_old:.3e}")
    assert e_new <= 1.5 * e_old + 1e-7, (e_new, e_old)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("rows", ROWS)
def test_plain_dwz_and_repeat_runs(rows, c):
    """packed_dx = 4 (fp32 dwz, max |dwz| as the by-product) and bit-equal repeats of every output, packed and plain."""
    _, ref = _inputs(rows, c)
    (a, ia), (b, ib) = _fused(rows, c, 1, False), _fused(rows, c, 1, False)
    assert ia and ib
    for k in a:
        same = a[k] == b[k] if k == "amax" else torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))
        assert same, f"{k} differs between two runs"
    old = _parent(rows, c, 1, False)
    e_new, e_old = _rel(a["dwz"], ref["dwz1"]), _rel(old["dwz"], ref["dwz1"])
    print(f"rows {rows} c {c} fp32 dwz: one walk {e_new:.3e} replaced sequence {e_old:.3e}")
    assert e_new <= 1.5 * e_old + 1e-7, (e_new, e_old)
    assert a["amax"] == float(a["dwz"].abs().max())
    (p, _), (q, iq) = _runs(rows, c, 1)[0], _fused(rows, c, 1, True)
    assert iq
    for k in p:
        same = p[k] == q[k] if k == "amax" else torch.equal(p[k].view(torch.int32), q[k].view(torch.int32))
        assert same, f"{k} (packed) differs between two runs"


def test_refusals():
    rows = 5
    t = torch.zeros(rows * 2052, device=DEV)
    v = torch.zeros(4 * 2052, device=DEV)
    ws = _ws(rows, 2052)

    def call(c, du, dz, w, x):
        return lib.glf_bn_res_ln_bwd_sums(dz.data_ptr(), w.data_ptr(), x.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(),
                                          v.data_ptr(), v.data_ptr(), v.data_ptr(), du.data_ptr(), v.data_ptr(), v.data_ptr(), v.data_ptr(),
                                          v.data_ptr(), v.data_ptr(), None, rows, c, 1, ws.data_ptr(), None)
    a, b, c_, d = (torch.zeros_like(t) for _ in range(4))
    assert call(2052, a, b, c_, d) != 0 and b"2048" in lib.glf_last_error()
    assert call(6, a, b, c_, d) != 0
    for alias in ((b, b, c_, d), (c_, b, c_, d), (d, b, c_, d)):
        assert call(8, *alias) != 0 and b"alias" in lib.glf_last_error()
    assert call(8, a, b, c_, d) == 0
    torch.cuda.synchronize()
