"""GPU: TPAVIModule's `gaussian` and `concatenate` pairwise modes.

The block is pinned to fixtures produced by executing the reference's own class (tests/golden/make_golden_tpavi_modes.py;
oracle.TPAVIModule restates `dot` and `embedded` only), at the gates test_gpu_model.test_tpavi_vs_golden applies to the other two
modes; the fused pairwise-ReLU kernels (csrc/attn_pair.hip) are checked on their own against float64 on the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import glfusion_ref as orc   # the checker (tests only)

DEV = "cuda"
MODES = ["gaussian", "concatenate"]


def close(a, b, tol):
    a = torch.as_tensor(a).detach().cpu().double()
    b = torch.as_tensor(b).detach().cpu().double()
    err = (a - b).abs()
    ok = bool((err <= tol + tol * b.abs()).all())
    print(f"    max abs err {float(err.max()):.3e} (max |ref| {float(b.abs().max()):.3e}, tol {tol:g}) -> {'ok' if ok else 'FAIL'}")
    return ok


def l2(a, truth) -> float:
    a = np.asarray(a, dtype=np.float64)
    t = np.asarray(truth, dtype=np.float64)
    return float(np.linalg.norm(a - t)) / max(float(np.linalg.norm(t)), 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the block against the reference's fixtures
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_tpavi_modes_vs_golden(golden_dir, mode, precision):
    """Body and gates of test_gpu_model.test_tpavi_vs_golden (z, z_eval 2e-5; dx 5e-5; running statistics 1e-6; gradient norms
    1e-4 max(1, norm); sampled gradient elements 1e-4; the W_z.0.bias rule), input range +-0.5 (see the fixture script)."""
    from glfusion_amd.models import TPAVIModule
    g = np.load(os.path.join(golden_dir, f"tpavi_{mode}.npz"))
    m = TPAVIModule(64, mode=mode)
    orc.closed_form_fill(m, salt=3)
    m = m.to(DEV).train()
    x = orc.closed_form_tensor((2, 64, 3, 6, 5), 101, -0.5, 0.5).to(DEV).requires_grad_(True)
    z, _ = m(x)
    assert tuple(z.shape) == (2, 64, 3, 6, 5)
    w = orc.closed_form_tensor(tuple(z.shape), 102, -1.0, 1.0).to(DEV)
    (z * w).sum().backward()
    print(f"  {mode} / {precision}: z"); ok_z = close(z, g["z"], 2e-5)
    print("  dx"); ok_dx = close(x.grad, g["dx"], 5e-5)
    print("  running mean / var"); ok_rs = close(m.W_z[1].running_mean, g["rm"], 1e-6) and close(m.W_z[1].running_var, g["rv"], 1e-6)
    norms = dict(zip(g["grad_names"].tolist(), g["grad_norms"].tolist()))
    bad = []
    for name, p in m.named_parameters():
        if norms[name] < 0:
            assert p.grad is None, name
            continue
        assert p.grad is not None, name
        gn = float(p.grad.double().norm())
        print(f"  grad {name}: norm {gn:.6e} (reference {norms[name]:.6e})")
        if name == "W_z.0.bias":          # exactly-zero true gradient (feeds a train-mode BN): rounding noise only
            if not gn <= 1e-4 * norms["W_z.0.weight"]:
                bad.append(name)
            continue
        if not abs(gn - norms[name]) <= 1e-4 * max(1.0, norms[name]):
            bad.append(name + ":norm")
        s = g["g:" + name]
        idx = np.unique(np.linspace(0, p.numel() - 1, num=min(33, p.numel())).astype(np.int64))
        if not close(p.grad.reshape(-1)[torch.from_numpy(idx).to(DEV)], s, 1e-4):
            bad.append(name + ":samples")
    m.eval()
    with torch.no_grad():
        print("  z_eval"); ok_ze = close(m(x.detach())[0], g["z_eval"], 2e-5)
    assert ok_z and ok_dx and ok_rs and ok_ze and not bad, (ok_z, ok_dx, ok_rs, ok_ze, bad)


def _odd_width_float64(golden_dir, mode, state):
    """z, dx, running mean / var and every parameter gradient of TPAVIModule(48, mode) in float64 on the +-1 input.  'embedded': the
    oracle's module, evaluated here; 'gaussian' (which the oracle does not restate): the reference's own class, evaluated in float64
    by tests/golden/make_golden_tpavi_modes.py."""
    if mode == "gaussian":
        g = np.load(os.path.join(golden_dir, "tpavi_gaussian_w48_f64.npz"))
        return {"z": g["z"], "dx": g["dx"], "rm": g["rm"], "rv": g["rv"]}, {k: g["g:" + k] for k in g["grad_names"].tolist()}
    ref = orc.TPAVIModule(48, mode=mode)
    ref.load_state_dict(state, strict=True)
    ref = ref.double().train()
    x = orc.closed_form_tensor((2, 48, 3, 6, 5), 101, -1.0, 1.0).double().requires_grad_(True)
    z, _ = ref(x)
    (z * orc.closed_form_tensor(tuple(z.shape), 102, -1.0, 1.0).double()).sum().backward()
    out = {"z": z.detach(), "dx": x.grad, "rm": ref.W_z[1].running_mean, "rv": ref.W_z[1].running_var}
    return out, {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("mode", ["gaussian", "embedded"])
def test_tpavi_materialised_odd_width_vs_float64(golden_dir, mode):
    """TPAVIModule(48, mode) (Ci = 24: no fused kernel, no frame groups -- the scores are materialised) at L = 90 under f32, against
    float64, at test_gpu_model.test_tpavi_vs_golden's gates: z 2e-5, dx 5e-5, running statistics 1e-6, gradient norms and elements
    1e-4, the W_z.0.bias rule."""
    from glfusion_amd import fusion, ops
    from glfusion_amd.models import TPAVIModule
    ops.set_precision("f32")
    if mode == "embedded":
        assert not fusion.fused_softmax_ok(24) and not fusion.chunked_softmax_ok(24, 90)
    else:
        assert not fusion.gaussian_chunked_ok(24)
    m = TPAVIModule(48, mode=mode)
    orc.closed_form_fill(m, salt=3)
    want, want_g = _odd_width_float64(golden_dir, mode, m.state_dict())
    m = m.to(DEV).train()
    x = orc.closed_form_tensor((2, 48, 3, 6, 5), 101, -1.0, 1.0).to(DEV).requires_grad_(True)
    z, _ = m(x)
    (z * orc.closed_form_tensor(tuple(z.shape), 102, -1.0, 1.0).to(DEV)).sum().backward()
    print(f"  {mode}: z"); ok = close(z, want["z"], 2e-5)
    print("  dx"); ok = close(x.grad, want["dx"], 5e-5) and ok
    print("  running mean / var"); ok = close(m.W_z[1].running_mean, want["rm"], 1e-6) and close(m.W_z[1].running_var, want["rv"], 1e-6) and ok
    bad = []
    for name, p in m.named_parameters():
        if name not in want_g:
            assert p.grad is None, name
            continue
        ref_g = torch.as_tensor(want_g[name]).double()
        gn, rn = float(p.grad.double().norm()), float(ref_g.norm())
        print(f"  grad {name}: norm {gn:.6e} (float64 {rn:.6e})")
        if name == "W_z.0.bias":          # exactly-zero true gradient (feeds a train-mode BN): rounding noise only
            if not gn <= 1e-4 * float(torch.as_tensor(want_g["W_z.0.weight"]).double().norm()):
                bad.append(name)
            continue
        if not abs(gn - rn) <= 1e-4 * max(1.0, rn) or not close(p.grad, ref_g, 1e-4):
            bad.append(name)
    assert ok and not bad, (ok, bad)


@pytest.mark.parametrize("prec", ["f32", "f16x3"])
def test_gaussian_frame_grouping_does_not_change_the_result(prec):
    """TPAVIModule(128, 'gaussian'), N = 3, L = 3 * 10 * 12 = 360 (rows padded to 384), train mode: one group of three frames against
    groups of two and one (a ragged last group).  No per-group quantity enters a frame's arithmetic under f32: bit for bit.  Under
    f16x3 the bound on |dP| that scales the split of dS is taken per group: output within 5e-5, dx, gradients and running statistics
    within 2e-4 relative L2 (the gates of test_chunked_split_fp16_softmax_attention_matches_fused_kernel)."""
    from glfusion_amd import fusion, ops
    from glfusion_amd.models import TPAVIModule
    res = {}
    old_bytes = fusion.CHUNK_BYTES
    ops.set_precision(prec)
    try:
        for frames, nbytes in ((3, old_bytes), (2, 2 * 360 * 384 * 4 + 1024)):
            fusion.CHUNK_BYTES = nbytes
            assert fusion.gaussian_chunked_ok(64) and fusion._frames_per_chunk(3, 360) == frames
            mod = TPAVIModule(128, mode="gaussian")
            _fill(mod, 61)
            mod = mod.to(DEV).train()
            x = (0.5 * torch.randn(3, 3, 10, 12, 128, generator=torch.Generator().manual_seed(611))).to(DEV).requires_grad_(True)
            z = mod.forward_nvhwc(x)
            z.backward(torch.randn(z.shape, generator=torch.Generator().manual_seed(77)).to(DEV))
            torch.cuda.synchronize()
            out = {"z": z.detach(), "dx": x.grad}
            out.update({"grad:" + k: p.grad for k, p in mod.named_parameters() if p.grad is not None})
            out.update({"buffer:" + k: b.detach().clone() for k, b in mod.named_buffers()})
            res[frames] = out
    finally:
        fusion.CHUNK_BYTES = old_bytes
        ops.set_precision("f32")
    one, two = res[3], res[2]
    assert set(one) == set(two)
    errs = {k: l2(two[k].double().cpu().numpy(), v.double().cpu().numpy()) for k, v in one.items()}
    print(f"  gaussian, groups of 2 + 1 against one group of 3 ({prec}):", {k: f"{e:.2e}" for k, e in errs.items()})
    if prec == "f32":
        for k, v in one.items():
            assert torch.equal(two[k], v), (k, errs[k])
        return
    top = max(float(v.norm()) for k, v in one.items() if k.startswith("grad:"))
    for k, v in one.items():
        if k.startswith("grad:") and not float(v.norm()) > 1e-5 * top:
            continue
        assert errs[k] <= (5e-5 if k == "z" else 2e-4), (k, errs[k])


# ---------------------------------------------------------------------------------------------------------------------------
# 2. parameters and buffers per mode are the reference's
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_tpavi_modes_state_dict_matches_reference(golden_dir, mode):
    from glfusion_amd.models import TPAVIModule
    g = np.load(os.path.join(golden_dir, f"tpavi_{mode}.npz"))
    m = TPAVIModule(64, mode=mode)
    sd = m.state_dict()
    ref_keys = [str(k) for k in g["keys"]]
    assert list(sd.keys()) == ref_keys
    assert [n for n, _ in m.named_parameters()] == g["grad_names"].tolist()
    assert [k for k in ref_keys if k not in set(g["grad_names"].tolist())] == [k for k, _ in m.named_buffers()]
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(d) for d in g["shape:" + k]), k
    if mode == "gaussian":
        assert not any(k.startswith(("theta", "phi", "W_f")) for k in sd)
    # a reference state dict (same keys, same shapes) loads strictly
    ref_sd = {k: torch.full(tuple(int(d) for d in g["shape:" + k]), 0.5).to(sd[k].dtype) for k in ref_keys}
    res = m.load_state_dict(ref_sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 64, 1, 2, 2), audio=torch.zeros(1, 1, 128))


# ---------------------------------------------------------------------------------------------------------------------------
# 3 / 4. glf_attn_pair_relu_fwd / _bwd against float64 on the host; write discipline; determinism
# ---------------------------------------------------------------------------------------------------------------------------
PAD = 37                 # floats after frames * L in a, b, da, db
LDX = 32                 # extra columns of the buffers g, y, dy, dg are slices of (slice = columns 16 .. 16 + Ci)
_pair_cache = {}


def _pair_problem(n, L, ci):
    """Inputs on a lattice: a_i, b_j integer multiples of 1/64 in [-1, 1], c = 1/128, so every s_ij is an odd multiple of
    1/128 -- exact in fp32 and never at the kink: the float64 reference has the identical mask.  Computed once per shape."""
    key = (n, L, ci)
    if key not in _pair_cache:
        rs = np.random.RandomState(1000 + 7 * n + 3 * L + ci)
        a = rs.randint(-64, 65, size=n * L).astype(np.float64) / 64.0
        b = rs.randint(-64, 65, size=n * L).astype(np.float64) / 64.0
        c = 1.0 / 128.0
        g = rs.uniform(-1, 1, size=(n, L, ci))
        dy = rs.uniform(-1, 1, size=(n, L, ci))
        g, dy = g.astype(np.float32).astype(np.float64), dy.astype(np.float32).astype(np.float64)
        s = a.reshape(n, L, 1) + b.reshape(n, 1, L) + c
        assert float(np.abs(s).min()) >= 1.0 / 128.0
        r = np.maximum(s, 0.0)
        ds = np.einsum("nic,njc->nij", dy, g) * (s > 0) / L
        ref = {"y": r @ g / L, "dg": r.transpose(0, 2, 1) @ dy / L, "da": ds.sum(2).reshape(-1), "db": ds.sum(1).reshape(-1),
               "dc": np.array([ds.sum()])}
        _pair_cache[key] = (a, b, c, g, dy, ref)
    return _pair_cache[key]


def _pair_run(n, L, ci):
    from glfusion_amd._lib import AttnPairParams, check, lib
    a, b, c, g, dy, ref = _pair_problem(n, L, ci)
    f32 = dict(dtype=torch.float32, device=DEV)
    nan = lambda *shape: torch.full(shape, float("nan"), **f32)
    ld = ci + LDX
    sl = slice(16, 16 + ci)
    ta, tb = nan(n * L + PAD), nan(n * L + PAD)
    ta[:n * L], tb[:n * L] = torch.from_numpy(a).to(**f32), torch.from_numpy(b).to(**f32)
    tc = torch.tensor([c], **f32)
    G, DY = nan(n * L, ld), nan(n * L, ld)
    G[:, sl], DY[:, sl] = torch.from_numpy(g.reshape(n * L, ci)).to(**f32), torch.from_numpy(dy.reshape(n * L, ci)).to(**f32)
    Y, DG = nan(n * L, ld), nan(n * L, ld)
    da, db, dc = nan(n * L + PAD), nan(n * L + PAD), nan(1 + PAD)
    pp = AttnPairParams()
    pp.frames, pp.L, pp.ci = n, L, ci
    pp.ldg = pp.ldy = pp.lddy = pp.lddg = ld
    nb = int(lib.glf_attn_pair_relu_workspace_bytes(C.byref(pp)))
    assert nb == n * ((L + 63) // 64) * L * 4
    ws = nan(nb // 4 + PAD)
    p = lambda t: C.c_void_p(t.data_ptr())
    check(lib.glf_attn_pair_relu_fwd(p(ta), p(tb), p(tc), p(G[:, sl]), p(Y[:, sl]), C.byref(pp), None), "fwd")
    check(lib.glf_attn_pair_relu_bwd(p(ta), p(tb), p(tc), p(G[:, sl]), p(DY[:, sl]), p(DG[:, sl]), p(da), p(db), p(dc), p(ws), nb,
                                     C.byref(pp), None), "bwd")
    torch.cuda.synchronize()
    return {"Y": Y, "DG": DG, "da": da, "db": db, "dc": dc, "ws": ws, "sl": sl}, ref


PAIR_SHAPES = [(2, 90, 64), (3, 64, 32), (1, 200, 96), (1, 130, 1024), (1, 40, 64)]


@pytest.mark.parametrize("n,L,ci", PAIR_SHAPES)
def test_attn_pair_relu_vs_float64(n, L, ci):
    """Relative L2 <= 2e-5 on y, dg, da, db, dc: the gate test_fused_softmax_attention_fwd_bwd applies to the same skeleton on the
    same MFMA.  g / dy / y / dg are column slices (row stride Ci + 32); L covers full, ragged and < 64 blocks."""
    from glfusion_amd import ops
    ops.set_precision("f32")
    out, ref = _pair_run(n, L, ci)
    sl = out["sl"]
    got = {"y": out["Y"][:, sl].reshape(n, L, ci), "dg": out["DG"][:, sl].reshape(n, L, ci), "da": out["da"][:n * L], "db": out["db"][:n * L],
           "dc": out["dc"][:1]}
    errs = {k: l2(v.cpu().numpy(), ref[k]) for k, v in got.items()}
    print(f"  pair relu ({n}, {L}, {ci}):", {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 2e-5 for e in errs.values()), errs


@pytest.mark.parametrize("n,L,ci", [(2, 90, 64), (1, 40, 64)])
def test_attn_pair_relu_write_discipline_and_determinism(n, L, ci):
    """Outputs pre-filled with NaN: every element inside is written (none survives), nothing outside the slices / beyond
    frames * L is touched, and a second run is bitwise equal."""
    out, _ = _pair_run(n, L, ci)
    sl = out["sl"]
    for k in ("Y", "DG"):
        t = out[k]
        assert bool(torch.isfinite(t[:, sl]).all()), k
        assert bool(torch.isnan(t[:, :sl.start]).all()) and bool(torch.isnan(t[:, sl.stop:]).all()), k
    for k in ("da", "db"):
        assert bool(torch.isfinite(out[k][:n * L]).all()) and bool(torch.isnan(out[k][n * L:]).all()), k
    assert bool(torch.isfinite(out["dc"][:1]).all()) and bool(torch.isnan(out["dc"][1:]).all())
    assert bool(torch.isnan(out["ws"][-PAD:]).all())
    again, _ = _pair_run(n, L, ci)
    for k in ("Y", "DG", "da", "db", "dc"):
        assert torch.equal(out[k].view(torch.int32), again[k].view(torch.int32)), k


def test_attn_pair_relu_argument_checks():
    from glfusion_amd._lib import AttnPairParams, lib
    assert C.sizeof(AttnPairParams) == lib.glf_sizeof_attn_pair_params()
    assert lib.glf_abi_version() == 7
    pp = AttnPairParams()
    pp.frames, pp.L, pp.ci = 1, 40, 48
    pp.ldg = pp.ldy = pp.lddy = pp.lddg = 48
    t = torch.zeros(40 * 48, device=DEV)
    p = C.c_void_p(t.data_ptr())
    assert lib.glf_attn_pair_relu_fwd(p, p, p, p, p, C.byref(pp), None) == -2             # GLF_ERR_UNSUPPORTED: Ci % 32
    pp.ci = 32
    assert lib.glf_attn_pair_relu_fwd(p, p, None, p, p, C.byref(pp), None) == -5          # GLF_ERR_NULL
    assert lib.glf_attn_pair_relu_bwd(p, p, p, p, p, p, p, p, p, p, 16, C.byref(pp), None) == -3      # GLF_ERR_WORKSPACE


# ---------------------------------------------------------------------------------------------------------------------------
# 5. nothing of size L x L for all frames
# ---------------------------------------------------------------------------------------------------------------------------
def _fill(mod, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if name.startswith("W_z.1") or name.startswith("norm_layer"):
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=gen))
            else:
                fan = max(1, p[0].numel()) if p.dim() > 1 else 1
                p.copy_(torch.randn(p.shape, generator=gen) * (fan ** -0.5 if p.dim() > 1 else 0.1))


def _block_peak(mode, x, seed):
    from glfusion_amd.models import TPAVIModule
    mod = TPAVIModule(2048, mode=mode)
    _fill(mod, seed)
    mod = mod.to(DEV).train()
    xin = x.clone().requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    z = mod.forward_nvhwc(xin)
    z.backward(torch.ones_like(z))
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    grads = {k: p.grad for k, p in mod.named_parameters() if p.grad is not None}
    assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(xin.grad).all())
    return peak, grads


def test_tpavi_modes_need_no_LxL_memory():
    """TPAVIModule(2048) forward + backward at N = 4, L = 3 * 28 * 28 = 2352 under f16x3: the peak stays within the `dot` block's on
    the same input + the chunk bound (gaussian: CHUNK_BYTES; concatenate: 64 MiB, the margin test_gpu_s16_attn.py uses)."""
    from glfusion_amd import fusion, ops
    ops.set_precision("f16x3")
    try:
        x = (0.05 * torch.randn(4, 3, 28, 28, 2048, generator=torch.Generator().manual_seed(91))).to(DEV)
        peaks = {m: _block_peak(m, x, 92)[0] for m in ("dot", "gaussian", "concatenate")}
    finally:
        ops.set_precision("f32")
    print("  peak above start (MiB):", {k: round(v / 2 ** 20) for k, v in peaks.items()})
    assert peaks["gaussian"] <= peaks["dot"] + fusion.CHUNK_BYTES, peaks
    assert peaks["concatenate"] <= peaks["dot"] + 64 * 2 ** 20, peaks


# ---------------------------------------------------------------------------------------------------------------------------
# 6. the model with both fusion blocks in the mode
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_model_with_mode_fusion_blocks(mode):
    """Global_and_Local(['1', '3']) with both fusion blocks replaced by TPAVIModule(2048, mode), N = 2, 112^2.  Eval forward under
    f16x3 against the same model under f32 at test_e2e_eval_vs_golden's gate on the masks (1e-4 absolute + relative); one train
    step gives finite, non-zero gradients for every fusion-block parameter the mode owns (align_channel: the dead audio branch)."""
    from glfusion_amd import ops
    from glfusion_amd.models import Global_and_Local, TPAVIModule
    views, n = ["1", "3"], 2
    model = Global_and_Local(views)
    model.global_attn = TPAVIModule(2048, mode=mode)
    model.local_attn = TPAVIModule(2048, mode=mode)
    orc.closed_form_fill(model, salt=1)
    orc.set_dropout(model, 0.0)
    model = model.to(DEV).eval()
    imgs = {v: t.to(DEV) for v, t in orc.closed_form_images(views, n).items()}
    outs = {}
    try:
        for prec in ("f32", "f16x3"):
            ops.set_precision(prec)
            with torch.no_grad():
                mask, mask_bb, _, _ = model(imgs)
            outs[prec] = ({v: mask[v].clone() for v in views}, {v: mask_bb[v].clone() for v in views})
        ok = True
        for v in views:
            print(f"  {mode} view {v}: mask, mask_bb (f16x3 vs f32)")
            ok = close(outs["f16x3"][0][v], outs["f32"][0][v], 1e-4) and ok
            ok = close(outs["f16x3"][1][v], outs["f32"][1][v], 1e-4) and ok
        model.train()
        mask, _, _, _ = model(imgs)
        sum(m.sum() for m in mask.values()).backward()
    finally:
        ops.set_precision("f32")
    for blk in ("global_attn", "local_attn"):
        for name, p in getattr(model, blk).named_parameters():
            if name.startswith("align_channel"):
                assert p.grad is None, name
                continue
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (blk, name)
            # gradients that are exactly zero in exact arithmetic (a constant added before a train-mode BatchNorm: W_z's bias, and
            # under 'gaussian' g's bias, since softmax rows sum to one) may come out as the exact value
            if name == "W_z.0.bias" or (mode == "gaussian" and name == "g.bias"):
                continue
            assert float(p.grad.abs().max()) > 0, (blk, name)
    assert ok
