"""CPU: TPAVIModule builds the reference's parameters for every pairwise mode (no GPU, no library call)."""
import os

import numpy as np
import pytest
import torch


@pytest.mark.parametrize("mode", ["gaussian", "concatenate"])
def test_tpavi_mode_parameters_match_reference_fixture(golden_dir, mode):
    from glfusion_amd.models import TPAVIModule
    g = np.load(os.path.join(golden_dir, f"tpavi_{mode}.npz"))
    m = TPAVIModule(64, mode=mode)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["keys"]]
    assert [n for n, _ in m.named_parameters()] == g["grad_names"].tolist()
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(int(d) for d in g["shape:" + k]), k
    ref_sd = {k: torch.zeros(tuple(int(d) for d in g["shape:" + k]), dtype=v.dtype) for k, v in sd.items()}
    m.load_state_dict(ref_sd, strict=True)
    assert hasattr(m, "theta") == (mode != "gaussian") and hasattr(m, "W_f") == (mode == "concatenate")
