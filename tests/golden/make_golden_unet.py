#!/usr/bin/env python3
"""Generate tests/golden/unet_baseline_unet.npz and unet_multiview_unet.npz by EXECUTING THE REFERENCE's baseline_unet and
multiview_unet (models/ours.py:2416-2625) on CPU (the import recipe and the helpers are make_golden.py's; only arrays are written).

Both models are built for views ["1", "3"], filled with oracle.closed_form_fill(salt=9) and run in eval() on two inputs:
closed_form_images(views, 2, 112, 112) (tag `a`: the training resolution, bottleneck 7 x 7) and closed_form_images(views, 3, 48, 32)
(tag `b`: bottleneck 3 x 2, L = 12 positions per frame in multiview_unet's fusion block).

Keys: `keys` (the state-dict keys in order), and per tag and view `mask_<tag>:<view>` -- a 20 011-point strided sample of the logit
map (make_golden.sample_idx) -- and `x5_<tag>:<view>`, a 4 099-point sample of the bottleneck features (the fourth output)."""
from __future__ import annotations

import os

import numpy as np
import torch

from make_golden import HERE, import_reference, orc, sample_idx, t2n

VIEWS = ["1", "3"]
INPUTS = {"a": (2, 112, 112), "b": (3, 48, 32)}


def main() -> None:
    torch.manual_seed(0)
    ours, _ = import_reference()
    for name in ("baseline_unet", "multiview_unet"):
        model = getattr(ours, name)(VIEWS)
        orc.closed_form_fill(model, salt=9)
        model.eval()
        d = {"keys": np.array(list(model.state_dict().keys()))}
        for tag, (n, h, w) in INPUTS.items():
            with torch.no_grad():
                out = model(orc.closed_form_images(VIEWS, n, h, w))
            assert out[1] is None and out[2] is None
            for v in VIEWS:
                m, x5 = out[0][v], out[3][v]
                d[f"mask_{tag}:{v}"] = t2n(m.reshape(-1)[torch.from_numpy(sample_idx(m.numel(), 20011))])
                d[f"x5_{tag}:{v}"] = t2n(x5.reshape(-1)[torch.from_numpy(sample_idx(x5.numel(), 4099))])
                print(name, tag, v, "|logit| mean %.3f, %.1f %% positive, |x5| max %.3f"
                      % (float(m.abs().mean()), 100.0 * float((m > 0).float().mean()), float(x5.abs().max())))
        np.savez_compressed(os.path.join(HERE, f"unet_{name}.npz"), **d)


if __name__ == "__main__":
    main()
