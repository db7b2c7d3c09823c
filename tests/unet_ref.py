"""Plain torch.nn restatement of the two U-Net comparison baselines (GLfusion/models/ours.py:2385-2625) with the reference's attribute
and state-dict names, for the tests: tests/test_unet_ref_cpu.py pins it to fixtures made by the reference's own classes
(tests/golden/unet_*.npz), the GPU tests compare train steps of the engine against it in float64.

`store`: a function applied to every tensor the engine keeps in memory in its storage precision -- convolution outputs and
BatchNorm(+ReLU) outputs, and inside the fusion block its projections, the W_z / BatchNorm / LayerNorm outputs.  The identity by
default; `bf16_store` makes the restatement an emulation of 16-bit storage (fp32 arithmetic, one bf16 rounding per stored tensor),
from which the bf16 gate of tests/test_gpu_unet.py is derived.  Pooling, up-sampling and concatenation copy values: no rounding.
The 5-channel logits stay fp32 under 16-bit storage and are not rounded."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from oracle import glfusion_ref as orc


def identity(t: torch.Tensor) -> torch.Tensor:
    return t


def bf16_store(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.bfloat16).to(t.dtype)


VIEWS = ["1", "3"]
INPUTS = {"a": (2, 112, 112), "b": (3, 48, 32)}          # the two inputs of tests/golden/make_golden_unet.py

# bf16_storage_deviation() as measured on the CPU (float32 torch), rounded down; tests/test_unet_ref_cpu.py recomputes it
BF16_DEVIATION = {"baseline_unet": {"a": 1.53e-2, "b": 1.67e-2}, "multiview_unet": {"a": 3.78e-2, "b": 1.63e-2}}


def bf16_storage_deviation(name: str) -> dict:
    """{input tag: largest deviation of the restatement's eval logits, relative to the largest logit, when every tensor the engine
    stores in bf16 is rounded to bf16 once (store=bf16_store), fp32 arithmetic otherwise}; closed_form_fill(salt=9) weights."""
    model = globals()[name](VIEWS)
    orc.closed_form_fill(model, salt=9)
    model.eval()
    dev = {}
    for tag, (n, h, w) in INPUTS.items():
        imgs = orc.closed_form_images(VIEWS, n, h, w)
        outs = []
        for store in (identity, bf16_store):
            model.store = store
            with torch.no_grad():
                outs.append(model(imgs)[0])
        dev[tag] = max(float((outs[1][v] - outs[0][v]).abs().max()) / float(outs[0][v].abs().max()) for v in VIEWS)
    return dev


class conv_block(nn.Module):
    def __init__(self, ch_in: int, ch_out: int) -> None:
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(ch_in, ch_out, 3, 1, 1, bias=True), nn.BatchNorm2d(ch_out), nn.ReLU(),
                                  nn.Conv2d(ch_out, ch_out, 3, 1, 1, bias=True), nn.BatchNorm2d(ch_out), nn.ReLU())

    def forward(self, x, store=identity):
        for i in (0, 3):
            x = store(F.relu(self.conv[i + 1](store(self.conv[i](x)))))
        return x


class up_conv(nn.Module):
    def __init__(self, ch_in: int, ch_out: int) -> None:
        super().__init__()
        self.up = nn.Sequential(nn.Upsample(scale_factor=2), nn.Conv2d(ch_in, ch_out, 3, 1, 1, bias=True), nn.BatchNorm2d(ch_out), nn.ReLU())

    def forward(self, x, store=identity):
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)           # nearest, scale 2
        return store(F.relu(self.up[2](store(self.up[1](x)))))


def fusion_dot(m: orc.TPAVIModule, x: torch.Tensor, store=identity) -> torch.Tensor:
    """TPAVIModule(mode='dot') (ours.py:863-915) on x [N,C,V,h,w] with the parameters of `m`."""
    n, ci = x.shape[0], m.inter_channels
    g = store(m.g(x)).reshape(n, ci, -1).transpose(1, 2)
    th = store(m.theta(x)).reshape(n, ci, -1).transpose(1, 2)
    ph = store(m.phi(x)).reshape(n, ci, -1)
    f = torch.matmul(th, ph)
    y = store(torch.matmul(f / f.shape[-1], g)).transpose(1, 2).reshape(n, ci, *x.shape[2:])
    z = store(m.W_z[1](store(m.W_z[0](y)))) + x
    return store(m.norm_layer(z.permute(0, 2, 3, 4, 1))).permute(0, 4, 1, 2, 3)


class baseline_unet(nn.Module):
    NAMES = ("Maxpool", "Conv1", "Conv2", "Conv3", "Conv4", "Conv5", "Up1", "Up2", "Up3", "Up4", "Up5",
             "Up_conv1", "Up_conv2", "Up_conv3", "Up_conv4", "Up_conv5", "Conv_1x1")
    store = staticmethod(identity)

    def __init__(self, view_num) -> None:
        super().__init__()
        self.view_num = view_num
        for name in self.NAMES:
            setattr(self, name, nn.ModuleDict())
        self._extra()
        widths = (1, 64, 128, 256, 512, 1024)
        for v in view_num:
            self.Maxpool[v] = nn.MaxPool2d(2, 2)
            for k in range(1, 6):
                getattr(self, f"Conv{k}")[v] = conv_block(widths[k - 1], widths[k])
            for k in range(5, 1, -1):
                getattr(self, f"Up{k}")[v] = up_conv(widths[k], widths[k - 1])
                getattr(self, f"Up_conv{k}")[v] = conv_block(widths[k], widths[k - 1])
            self.Conv_1x1[v] = nn.Conv2d(64, 5, 1)

    def _extra(self) -> None:
        pass

    def encode(self, v, x):
        skips = []
        f = self.Conv1[v](x, self.store)
        for k in range(2, 6):
            skips.append(f)
            f = getattr(self, f"Conv{k}")[v](self.Maxpool[v](f), self.store)
        return skips, f

    def decode(self, v, skips, f):
        for k in range(5, 1, -1):
            f = getattr(self, f"Up_conv{k}")[v](torch.cat((skips[k - 2], getattr(self, f"Up{k}")[v](f, self.store)), dim=1), self.store)
        return self.Conv_1x1[v](f)

    def fuse(self, x5):
        return x5

    def forward(self, x):
        enc = {v: self.encode(v, x[v]) for v in self.view_num}
        x5 = self.fuse({v: enc[v][1] for v in self.view_num})
        return {v: self.decode(v, enc[v][0], x5[v]) for v in self.view_num}, None, None, x5


class multiview_unet(baseline_unet):
    def _extra(self) -> None:
        self.global_attn = orc.TPAVIModule(1024, mode="dot")

    def fuse(self, x5):
        z = fusion_dot(self.global_attn, torch.stack([x5[v] for v in self.view_num], dim=2), self.store)
        return {v: z[:, :, i] for i, v in enumerate(self.view_num)}
