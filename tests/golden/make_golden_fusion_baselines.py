#!/usr/bin/env python3
"""Generate tests/golden/fusion_early_fusion.npz, fusion_late_fusion.npz and fusion_MLP_fusion.npz by EXECUTING THE REFERENCE's
early_fusion, late_fusion and MLP_fusion (models/ours.py:2251-2383, 1044-1107) on CPU (the import recipe and the helpers are
make_golden.py's; only arrays are written).

Each model is built for views ["1", "3", "4"], filled with oracle.closed_form_fill(salt=11) and run in eval() on two inputs:
closed_form_images(views, 2, 112, 112) (tag `a`: the training resolution, 28 x 28 feature maps) and closed_form_images(views, 3, 64, 48)
(tag `b`: 16 x 12 feature maps).  early_fusion overwrites the entries of the dict it is given, so every call gets a fresh one.

Keys: `keys` (the state-dict keys in order), and per tag and view `mask_<tag>:<view>` -- a 20 011-point strided sample of the logit
map (make_golden.sample_idx) -- and `f4_<tag>:<view>`, a 4 099-point sample of the layer-4 features (the second output)."""
from __future__ import annotations

import os

import numpy as np
import torch

from make_golden import HERE, import_reference, orc, sample_idx, t2n

VIEWS = ["1", "3", "4"]
INPUTS = {"a": (2, 112, 112), "b": (3, 64, 48)}
NAMES = ("early_fusion", "late_fusion", "MLP_fusion")


def main() -> None:
    torch.manual_seed(0)
    ours, _ = import_reference()
    for name in NAMES:
        model = getattr(ours, name)(VIEWS)
        orc.closed_form_fill(model, salt=11)
        model.eval()
        d = {"keys": np.array(list(model.state_dict().keys()))}
        print(name, len(d["keys"]), "keys,", sum(p.numel() for p in model.parameters()), "parameters")
        for tag, (n, h, w) in INPUTS.items():
            with torch.no_grad():
                out = model(dict(orc.closed_form_images(VIEWS, n, h, w)))
            assert out[2] is None and out[3] is None
            for v in VIEWS:
                m, f4 = out[0][v], out[1][v]
                d[f"mask_{tag}:{v}"] = t2n(m.reshape(-1)[torch.from_numpy(sample_idx(m.numel(), 20011))])
                d[f"f4_{tag}:{v}"] = t2n(f4.reshape(-1)[torch.from_numpy(sample_idx(f4.numel(), 4099))])
                print(name, tag, v, "|logit| mean %.3f, %.1f %% positive, |f4| max %.3f"
                      % (float(m.abs().mean()), 100.0 * float((m > 0).float().mean()), float(f4.abs().max())))
        np.savez_compressed(os.path.join(HERE, f"fusion_{name}.npz"), **d)
        del model


if __name__ == "__main__":
    main()
