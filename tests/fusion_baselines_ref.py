"""Plain torch.nn restatement of the three classical fusion baselines (GLfusion/models/ours.py: early_fusion 2251-2315, late_fusion
2317-2383, MLP_fusion 1044-1107) with the reference's attribute and state-dict names, assembled from the oracle's
deeplabv3_resnet50_iekd and TPAVIModule, for the tests: tests/test_fusion_baselines_ref_cpu.py pins it to fixtures made by the
reference's own classes (tests/golden/fusion_*.npz), the GPU tests compare train steps of the engine against it in float64.

Unlike the reference's early_fusion, forward leaves the caller's dict as it was."""
from __future__ import annotations

import copy

import torch
import torch.nn.functional as F
from torch import nn

from oracle import glfusion_ref as orc

VIEWS = ["1", "3", "4"]
INPUTS = {"a": (2, 112, 112), "b": (3, 64, 48)}          # the two inputs of tests/golden/make_golden_fusion_baselines.py
NAMES = ("early_fusion", "late_fusion", "MLP_fusion")
SALT = 11


class _FusionBaseline(nn.Module):
    fc_channels = 0

    def __init__(self, view_num, test_view=("1", "2", "3", "4")) -> None:
        super().__init__()
        self.view_num, self.test_view = view_num, test_view
        self.network = orc.deeplabv3_resnet50_iekd(pretrained=False, aux_loss=False)
        for name in ("init_block", "layer1", "layer2", "layer3", "layer4", "fc", "classifier"):
            setattr(self, name, nn.ModuleDict())
        bb = self.network.backbone
        for v in view_num:
            self.init_block[v] = copy.deepcopy(nn.Sequential(bb["conv1"], bb["bn1"], bb["relu"], bb["maxpool"]))
            for l in ("layer1", "layer2", "layer3", "layer4"):
                getattr(self, l)[v] = copy.deepcopy(bb[l])
            self.fc[v] = nn.Conv2d(self.fc_channels * len(view_num), self.fc_channels, kernel_size=1)
            self.classifier[v] = copy.deepcopy(self.network.classifier)
            self.classifier[v][-1] = nn.Conv2d(256, 5, kernel_size=1)
        self.non_local = orc.TPAVIModule(2048, mode="dot")          # registered, never called

    def encode(self, v, xv):
        f = self.init_block[v](xv)
        for l in ("layer1", "layer2", "layer3", "layer4"):
            f = getattr(self, l)[v](f)
        return f

    def mix(self, per_view):
        cat = torch.cat([per_view[v] for v in self.view_num], dim=1)
        return {v: self.fc[v](cat) for v in self.view_num}

    def up(self, m, hw):
        return F.interpolate(m, size=hw, mode="bilinear", align_corners=False)


class early_fusion(_FusionBaseline):
    fc_channels = 1

    def forward(self, x):
        hw = x[self.view_num[0]].shape[-2:]
        mixed = self.mix(x)
        f4 = {v: self.encode(v, mixed[v]) for v in self.view_num}
        return {v: self.up(self.classifier[v](f4[v]), hw) for v in self.view_num}, f4, None, None


class late_fusion(_FusionBaseline):
    fc_channels = 5

    def forward(self, x):
        hw = x[self.view_num[0]].shape[-2:]
        f4 = {v: self.encode(v, x[v]) for v in self.view_num}
        mixed = self.mix({v: self.classifier[v](f4[v]) for v in self.view_num})
        return {v: self.up(mixed[v], hw) for v in self.view_num}, f4, None, None


class MLP_fusion(_FusionBaseline):
    fc_channels = 2048

    def forward(self, x):
        hw = x[self.view_num[0]].shape[-2:]
        f4 = {v: self.encode(v, x[v]) for v in self.view_num}
        fused = self.mix(f4)
        return {v: self.up(self.classifier[v](fused[v]), hw) for v in self.view_num}, f4, None, None
