"""CPU: the U-Net baselines' restatement (tests/unet_ref.py) against the fixtures made by the reference's own baseline_unet /
multiview_unet (tests/golden/make_golden_unet.py), and the engine's classes against the reference's state-dict keys."""
import os

import numpy as np
import pytest
import torch

from oracle import glfusion_ref as orc

import unet_ref

VIEWS = ["1", "3"]
INPUTS = {"a": (2, 112, 112), "b": (3, 48, 32)}
NAMES = ("baseline_unet", "multiview_unet")


def sample(t: torch.Tensor, k: int) -> torch.Tensor:
    flat = t.detach().reshape(-1)
    return flat[torch.from_numpy(np.unique(np.linspace(0, flat.numel() - 1, num=min(k, flat.numel())).astype(np.int64)))]


@pytest.mark.parametrize("name", NAMES)
def test_fixture_holds_the_reference_keys(golden_dir, name):
    g = np.load(os.path.join(golden_dir, f"unet_{name}.npz"))
    keys = g["keys"].tolist()
    assert len(keys) == {"baseline_unet": 312, "multiview_unet": 329}[name]
    assert keys[0] == "Conv1.1.conv.0.weight" and ("global_attn.align_channel.weight" in keys) == (name == "multiview_unet")
    assert os.path.getsize(os.path.join(golden_dir, f"unet_{name}.npz")) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference(golden_dir, name):
    """Logit samples within 1e-5 of the largest logit (the reference's own fp32-vs-fp64 difference is <= 3.3e-6), x5 likewise."""
    g = np.load(os.path.join(golden_dir, f"unet_{name}.npz"))
    model = getattr(unet_ref, name)(VIEWS)
    assert list(model.state_dict().keys()) == g["keys"].tolist()
    orc.closed_form_fill(model, salt=9)
    model.eval()
    for tag, (n, h, w) in INPUTS.items():
        with torch.no_grad():
            out = model(orc.closed_form_images(VIEWS, n, h, w))
        assert out[1] is None and out[2] is None
        for v in VIEWS:
            assert tuple(out[0][v].shape) == (n, 5, h, w) and tuple(out[3][v].shape) == (n, 1024, h // 16, w // 16)
            for got, want in ((sample(out[0][v], 20011), g[f"mask_{tag}:{v}"]), (sample(out[3][v], 4099), g[f"x5_{tag}:{v}"])):
                want = torch.from_numpy(want)
                err = float((got - want).abs().max())
                assert err <= 1e-5 * float(want.abs().max()), (tag, v, err, float(want.abs().max()))


@pytest.mark.parametrize("name", NAMES)
def test_bf16_storage_deviation_is_what_the_gpu_gate_assumes(name):
    """unet_ref.BF16_DEVIATION (from which tests/test_gpu_unet.py takes its 16-bit-storage limit) re-measured: the largest of
    millions of rounding events, so another CPU's fp32 convolutions may move it a little -- within a quarter either way."""
    got = unet_ref.bf16_storage_deviation(name)
    for tag, want in unet_ref.BF16_DEVIATION[name].items():
        assert 0.8 * want <= got[tag] <= 1.25 * want, (name, tag, got[tag], want)


@pytest.mark.parametrize("name", NAMES)
def test_engine_classes_have_the_reference_keys(golden_dir, name):
    import glfusion_amd.models as M
    g = np.load(os.path.join(golden_dir, f"unet_{name}.npz"))
    model = getattr(M, name)(VIEWS)
    sd = model.state_dict()
    assert list(sd.keys()) == g["keys"].tolist()
    ref = getattr(unet_ref, name)(VIEWS).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(v.shape) for k, v in ref.items()}
    assert type(M.conv_block(4, 8).conv[0]).__module__.startswith("glfusion_amd") and isinstance(M.up_conv(8, 4).up[0], torch.nn.Upsample)


def test_engine_models_refuse_cpu_tensors_and_ragged_sizes():
    import glfusion_amd.models as M
    m = M.baseline_unet(["1"])
    with pytest.raises(RuntimeError, match="multiples of 16"):
        m({"1": torch.zeros(1, 1, 40, 32)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m({"1": torch.zeros(1, 1, 32, 32)})


def test_layers_keep_their_refusals():
    from glfusion_amd.models import layers
    x = torch.zeros(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="on the path"):
        layers.MaxPool2d(2, 1).forward_nhwc(x)
    with pytest.raises(RuntimeError, match="on the path"):
        layers.MaxPool2d(2, 2, ceil_mode=True).forward_nhwc(x)
    with pytest.raises(RuntimeError, match="on the path"):
        layers.Upsample(scale_factor=3).forward_nhwc(x)
    with pytest.raises(RuntimeError, match="on the path"):
        layers.Upsample(scale_factor=2, mode="bilinear").forward_nhwc(x)
    with pytest.raises(RuntimeError, match="Cin=1 is not on the path"):
        layers.Conv2d(1, 64, 3, padding=0).forward_nhwc(torch.zeros(1, 4, 4, 1))
    with pytest.raises(RuntimeError, match="Cin=1 is not on the path"):
        layers.Conv2d(1, 64, 5, padding=2).forward_nhwc(torch.zeros(1, 4, 4, 1))


def test_workspace_query_of_the_entry_convolution():
    """Host-only: one [10][Cout] block of partial sums per 1024 pixels."""
    from glfusion_amd._lib import lib
    q = lib.glf_conv3x3_c1_wgrad_workspace
    assert q(1, 1, 1023, 64) == 640 and q(1, 32, 32, 64) == 640 and q(1, 1, 1025, 64) == 1280
    assert q(2, 48, 32, 64) == 3 * 640 and q(0, 4, 4, 64) == 0
