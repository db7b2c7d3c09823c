"""Views with different numbers of frames: the model's view stack refuses them (its copies take every view at the first one's
extents), and the per-epoch validation, whose per-view clip windows may be cut short at the end of a volume, feeds the model the
views' common leading frames."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_stack_views_refuses_views_of_different_shapes():
    from glfusion_amd import ops
    a, b = torch.zeros(4, 2, 2, 32, device=DEV), torch.zeros(3, 2, 2, 32, device=DEV)
    with pytest.raises(RuntimeError, match="must have one shape"):
        ops.stack_views([a, b])
    with pytest.raises(RuntimeError, match="must have one shape"):
        ops.stack_views([b, a])
    assert tuple(ops.stack_views([a, a.clone()]).shape) == (4, 2, 2, 2, 32)


def test_validation_with_clip_windows_of_different_lengths(tmp_path, monkeypatch):
    from glfusion_amd import data
    from glfusion_amd.engine import Trainer
    views = ["1", "4"]
    infos = data.synthetic_infos(views, 3, clip_length=6, device="cpu", seed=2)
    cfg = {"train": {"view_num": views, "test_view": views, "num_epochs": 1, "batch_size": 2, "iters_per_epoch": 1, "clip_length": 6,
                     "save_dir": str(tmp_path), "validate_every_epoch": False},
           "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "weight_decay": 1e-5}}}
    t = Trainer(cfg)
    drawn, fed = [], []
    real_item = data.SegPAHDataset.__getitem__

    def item(self, index):
        out = real_item(self, index)
        drawn.append(out[0].shape[-1])
        return out
    monkeypatch.setattr(data.SegPAHDataset, "__getitem__", item)
    real_forward = t.model.forward

    def forward(imgs, *a, **kw):
        fed.append([imgs[v].shape[0] for v in views])
        return real_forward(imgs, *a, **kw)
    t.model.forward = forward
    random.seed(3)
    val = t.validation_and_test(net_root=None, infos=infos, raw_data=False, val_list=("0_0",), test_list=("0_1", "0_2"))
    assert 0.0 <= val <= 1.0
    pairs = list(zip(drawn[0::2], drawn[1::2]))
    print(f"frames drawn per clip and view {pairs}, fed {fed}")
    assert len(fed) == 3 and any(a != b for a, b in pairs)                   # the case is met: some clip's windows differ
    assert fed == [[min(p), min(p)] for p in pairs]
    for split in ("Inner-val", "Inner-test"):
        for v in views:
            m = t.validation_report[split][v]
            assert all(0.0 <= x <= 1.0 for x in m["metrics"]) and len(m["part_dice"]) == 5 and m["loss"] > 0
