#!/usr/bin/env python3
"""Generate tests/golden/tpavi_gaussian.npz and tpavi_concatenate.npz by EXECUTING THE REFERENCE's TPAVIModule on CPU
(the import recipe and the helpers are make_golden.py's; only arrays are written).

Key layout: that of tpavi_dot.npz -- z, dx, grad_names, grad_norms, g:<name> samples, rm, rv, z_eval -- plus the state-dict
keys and shapes of the reference module (`keys`, `shape:<key>`), which tests/test_gpu_tpavi_modes.py pins the module to.

The input range is +-0.5, not the +-1 of the other TPAVI fixtures: at +-1 the gaussian softmax of x x^T is one-hot (mean row
maximum 0.99999) and would not exercise the softmax (at +-0.5: 0.65), and the smallest |s_ij| of the concatenate scores is 3e-5
(at +-0.5: 2.0e-4, two orders above any split-fp16 rounding, so no ReLU mask can differ between arithmetics).

tpavi_gaussian_w48_f64.npz (argument `w48` writes it alone): the reference's class at width 48 (Ci = 24, the width at which the
engine materialises the scores), evaluated in float64 on the +-1 input of the other TPAVI fixtures, with every gradient in full."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

from make_golden import HERE, grads_summary, import_reference, orc, t2n


def odd_width(ours) -> None:
    m = ours.TPAVIModule(in_channels=48, mode="gaussian")
    orc.closed_form_fill(m, salt=3)
    m = m.double().train()
    x = orc.closed_form_tensor((2, 48, 3, 6, 5), 101, -1.0, 1.0).double().requires_grad_(True)
    z, _ = m(x)
    (z * orc.closed_form_tensor(tuple(z.shape), 102, -1.0, 1.0).double()).sum().backward()
    d = {"z": t2n(z), "dx": t2n(x.grad), "rm": t2n(m.W_z[1].running_mean), "rv": t2n(m.W_z[1].running_var),
         "grad_names": np.array([k for k, p in m.named_parameters() if p.grad is not None])}
    d.update({"g:" + k: t2n(p.grad) for k, p in m.named_parameters() if p.grad is not None})
    np.savez_compressed(os.path.join(HERE, "tpavi_gaussian_w48_f64.npz"), **d)
    print("tpavi gaussian width 48 (float64): |z|max", float(z.abs().max()))


def main() -> None:
    torch.manual_seed(0)
    ours, _ = import_reference()
    odd_width(ours)
    if sys.argv[1:] == ["w48"]:
        return
    for mode in ("gaussian", "concatenate"):
        m = ours.TPAVIModule(in_channels=64, mode=mode)
        orc.closed_form_fill(m, salt=3)
        m.train()
        x = orc.closed_form_tensor((2, 64, 3, 6, 5), 101, -0.5, 0.5).requires_grad_(True)
        z, _ = m(x)
        w = orc.closed_form_tensor(tuple(z.shape), 102, -1.0, 1.0)
        (z * w).sum().backward()
        names, norms, samples = grads_summary(m)
        d = {"z": t2n(z), "dx": t2n(x.grad), "grad_names": np.array(names), "grad_norms": norms,
             "rm": t2n(m.W_z[1].running_mean), "rv": t2n(m.W_z[1].running_var)}
        d.update({"g:" + k: v for k, v in samples.items()})
        sd = m.state_dict()
        d["keys"] = np.array(list(sd.keys()))
        d.update({"shape:" + k: np.array(tuple(v.shape), dtype=np.int64) for k, v in sd.items()})
        m.eval()
        with torch.no_grad():
            d["z_eval"] = t2n(m(x.detach())[0])
        np.savez_compressed(os.path.join(HERE, f"tpavi_{mode}.npz"), **d)
        print("tpavi", mode, "|z|max", float(z.abs().max()), "grad norms", dict(zip(names, np.round(norms, 6).tolist())))


if __name__ == "__main__":
    main()
