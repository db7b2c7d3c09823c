"""fusion.TAIL_BWD_FUSED: the fusion block's backward with the tail walked once (glf_bn_res_ln_bwd_sums + the apply half of
glf_bn_bwd) and the stacked projection's bias gradient read off the pass that packs dqkv (glf_split_f16_packed_colsum), against the
separate passes (switch off) -- one TPAVIModule(64, 'dot') forward + backward at N = 2, V = 3, h = w = 5, train and eval.

Yardstick (test_gpu_aspp_centre.py's): against the oracle's float64 block on the same closed-form inputs, the relative L2 error of
every parameter gradient and of x.grad with the switch on is <= 1.5 x the error with it off + 1e-7; both are printed.  W_z.0.bias in
train mode has the true gradient 0 (the bias feeds a train-mode BatchNorm), a relative error does not exist: both settings must stay
within test_gpu_model.test_tpavi_vs_golden's gate for it, 1e-4 of the norm of W_z.0.weight's gradient."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import glfusion_ref as orc   # the checker (tests only)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SHAPE = (2, 64, 3, 5, 5)
SPIED = ("glf_bn_res_ln_bwd", "glf_bn_res_ln_bwd_sums", "glf_bn_bwd", "glf_colsum", "glf_split_f16_packed", "glf_split_f16_packed_colsum")

_ORACLE = {}


def _oracle(training):
    if training not in _ORACLE:
        ref = orc.TPAVIModule(64, mode="dot")
        orc.closed_form_fill(ref, salt=5)
        state = {k: v.clone() for k, v in ref.state_dict().items()}
        ref = ref.double().train(training)
        x = orc.closed_form_tensor(SHAPE, 201, -1.0, 1.0).double().requires_grad_(True)
        z, _ = ref(x)
        (z * orc.closed_form_tensor(tuple(z.shape), 202, -1.0, 1.0).double()).sum().backward()
        grads = {k: p.grad.detach() for k, p in ref.named_parameters() if p.grad is not None}
        grads["x"] = x.grad.detach()
        _ORACLE[training] = (state, grads)
    return _ORACLE[training]


def _run(prec, fused, training):
    """-> {name: gradient}, [(entry point, arguments)] of the spied library calls made during backward."""
    from glfusion_amd import fusion, ops
    from glfusion_amd._lib import lib
    from glfusion_amd.models import TPAVIModule
    state, _ = _oracle(training)
    calls = []
    real = {name: getattr(lib, name) for name in SPIED}

    def spy(name):
        def f(*a):
            calls.append((name, a))
            return real[name](*a)
        return f
    keep = fusion.TAIL_BWD_FUSED
    try:
        fusion.TAIL_BWD_FUSED = fused
        with ops.precision_scope(prec):
            m = TPAVIModule(64, mode="dot")
            m.load_state_dict(state, strict=True)
            m = m.to(DEV).train(training)
            x = orc.closed_form_tensor(SHAPE, 201, -1.0, 1.0).to(DEV).requires_grad_(True)
            z, _ = m(x)
            loss = (z * orc.closed_form_tensor(tuple(z.shape), 202, -1.0, 1.0).to(DEV)).sum()
            for name in SPIED:
                setattr(lib, name, spy(name))
            loss.backward()
            torch.cuda.synchronize()
            ops.reset_weight_images()
    finally:
        fusion.TAIL_BWD_FUSED = keep
        for name in SPIED:
            if name in lib.__dict__:
                delattr(lib, name)
    out = {k: p.grad.detach().cpu() for k, p in m.named_parameters() if p.grad is not None}
    out["x"] = x.grad.detach().cpu()
    return out, calls


def _rel(a, ref):
    return float((a.double().reshape(-1) - ref.reshape(-1)).norm()) / max(float(ref.norm()), 1e-300)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_block_backward_switch_on_against_off(prec, training):
    _, want = _oracle(training)
    on, calls_on = _run(prec, True, training)
    off, calls_off = _run(prec, False, training)
    rows, c, c3 = SHAPE[0] * SHAPE[2] * SHAPE[3] * SHAPE[4], 64, 3 * 32
    names_on, names_off = [n for n, _ in calls_on], [n for n, _ in calls_off]
    # on: one walk, then the apply half alone (packed_dx 3 where dwz is written packed, 4 where it stays fp32)
    assert names_on.count("glf_bn_res_ln_bwd_sums") == 1 and "glf_bn_res_ln_bwd" not in names_on
    bn_on = [a for n, a in calls_on if n == "glf_bn_bwd"]
    packed_dwz = prec == "f16x3" and training
    assert len(bn_on) == 1 and bn_on[0][22] == (3 if packed_dwz else 4)
    colsum_cols_on = [a[4] for n, a in calls_on if n == "glf_colsum"]
    if prec == "f16x3":
        assert c3 not in colsum_cols_on and names_on.count("glf_split_f16_packed_colsum") == 1, "dqkv is still summed by its own pass"
    else:
        assert c3 in colsum_cols_on and "glf_split_f16_packed_colsum" not in names_on          # exact fp32 keeps colsum
    # off: the separate passes
    assert names_off.count("glf_bn_res_ln_bwd") == 1 and "glf_bn_res_ln_bwd_sums" not in names_off
    assert "glf_split_f16_packed_colsum" not in names_off and c3 in [a[4] for n, a in calls_off if n == "glf_colsum"]
    bn_off = [a for n, a in calls_off if n == "glf_bn_bwd"]
    assert len(bn_off) == 1 and bn_off[0][22] == int(packed_dwz)
    assert set(on) == set(off) == set(want), set(on) ^ set(want)
    wnorm = float(want["W_z.0.weight"].norm())
    for key, ref in want.items():
        if key == "W_z.0.bias" and training:
            n_on, n_off = float(on[key].double().norm()) / wnorm, float(off[key].double().norm()) / wnorm
            print(f"{prec} train {key}: |gradient| / |dW_z| on {n_on:.3e} off {n_off:.3e} (true value 0)")
            assert n_on <= 1e-4 and n_off <= 1e-4, (n_on, n_off)
            continue
        e_on, e_off = _rel(on[key], ref), _rel(off[key], ref)
        print(f"{prec} training {training} {key}: on {e_on:.3e} off {e_off:.3e}")
        assert e_on <= 1.5 * e_off + 1e-7, (key, e_on, e_off)


def test_environment_switch():
    """GLF_TAIL_BWD_FUSED=0 selects the separate passes at import; unset or 1, the one-walk route."""
    code = "from glfusion_amd import fusion; print(int(fusion.TAIL_BWD_FUSED))"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "GLF_TAIL_BWD_FUSED"}
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    for value, want in ((None, "1"), ("0", "0"), ("1", "1")):
        e = dict(env) if value is None else dict(env, GLF_TAIL_BWD_FUSED=value)
        got = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, check=True).stdout.split("\n")[-2]
        assert got == want, (value, got)
