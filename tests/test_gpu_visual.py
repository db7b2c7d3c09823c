"""GPU: the visual mode (glf_render_labels, glf_restore_labels, Trainer.test_visualize) against its restatement in numpy / torch
CPU ops (tests/visual_ref.py, pinned to main.py:606-612 by tests/test_visual_cpu.py).  Everything is integer or index work: every
comparison is torch.equal / array_equal, there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import visual_ref as V
from oracle import glfusion_ref as orc   # the checker (tests only)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 1, 1), (3, 5, 7), (2, 9, 65), (2, 112, 112)]                  # one pixel; odd; a ragged row past one block; the model's
PAL1 = ((9, 8, 7, 6), (1, 2, 3, 4))
PAL8 = tuple((10 * k + 1, 255 - 20 * k, 7 * k, 255 - k) for k in range(9))


def _logits(n, c, h, w):
    g = torch.Generator().manual_seed(n * 1000 + c * 100 + h + w)
    return V.plant(torch.randn(n, c, h, w, generator=g) * 3)


def _frames(n, h, w):
    """level / 255.0 for the integer levels 0..255 in turn, plus -0.2, 1.3 and NaN where there is room."""
    f = (torch.arange(n * h * w) % 256).float() / 255.0
    for k, v in enumerate((-0.2, 1.3, float("nan"))):
        if f.numel() > 300 + k:
            f[260 + 7 * k] = v
    return f.view(n, 1, h, w)


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_render_labels_matches_restatement(n, h, w):
    from glfusion_amd import data
    x = _logits(n, 5, h, w)
    assert not bool(((x > 0) & (x < 1e-6)).any())
    want = V.labels_ref(x)
    labels, rgba = data.render_labels(x.to(DEV))
    assert labels.dtype == torch.uint8 and tuple(labels.shape) == (n, h, w) and rgba.dtype == torch.uint8 and tuple(rgba.shape) == (n, h, w, 4)
    assert torch.equal(labels.cpu(), want)
    assert torch.equal(rgba.cpu(), V.rgba_ref(want, data.PALETTE))
    if h * w > 20:
        assert set(want.unique().tolist()) == {0, 1, 2, 3, 4, 5}            # the fixture is not degenerate
    # a non-contiguous view goes through _contig
    xt = x.permute(0, 1, 3, 2).contiguous().to(DEV).permute(0, 1, 3, 2)
    assert torch.equal(data.render_labels(xt)[0].cpu(), want)


@pytest.mark.parametrize("c,palette", [(1, PAL1), (8, PAL8)])
def test_render_labels_other_channel_counts(c, palette):
    from glfusion_amd import data
    x = _logits(2, c, 9, 65)
    want = V.labels_ref(x)
    labels, rgba = data.render_labels(x.to(DEV), palette=palette)
    assert torch.equal(labels.cpu(), want) and int(want.max()) == c
    assert torch.equal(rgba.cpu(), V.rgba_ref(want, palette))
    with pytest.raises(ValueError, match="palette"):
        data.render_labels(x.to(DEV))                                        # six rows do not fit c + 1
    if c == 8:
        with pytest.raises(RuntimeError, match="at most 8"):
            data.render_labels(torch.zeros(1, 9, 2, 2, device=DEV), palette=PAL8 + ((0, 0, 0, 0),))


def test_render_labels_only_and_rgba_only():
    """Either output may be null: the other one is written all the same, and nothing else is (guard bytes around both)."""
    from glfusion_amd import data
    from glfusion_amd._lib import check, lib
    from glfusion_amd.ops import _p, _stream
    n, h, w = 2, 9, 65
    x = _logits(n, 5, h, w)
    want = V.labels_ref(x)
    xd = x.to(DEV)
    pal = (C.c_uint8 * 24)(*[v for row in data.PALETTE for v in row])
    guard = 64
    lab = torch.full((n * h * w + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    pix = torch.full((n * h * w * 4 + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    check(lib.glf_render_labels(_p(xd), None, _p(lab[guard:]), None, n, 5, h, w, None, 255, _stream()), "labels only")
    check(lib.glf_render_labels(_p(xd), None, None, _p(pix[guard:]), n, 5, h, w, pal, 255, _stream()), "rgba only")
    lab, pix = lab.cpu(), pix.cpu()
    assert torch.equal(lab[guard:-guard].view(n, h, w), want)
    assert torch.equal(pix[guard:-guard].view(n, h, w, 4), V.rgba_ref(want, data.PALETTE))
    for buf in (lab, pix):
        assert bool((buf[:guard] == 0xAB).all()) and bool((buf[-guard:] == 0xAB).all())
    with pytest.raises(RuntimeError, match="4-byte aligned"):
        check(lib.glf_render_labels(_p(xd), None, None, _p(pix.to(DEV)[guard + 1:]), n, 5, h, w, pal, 255, _stream()), "misaligned")


@pytest.mark.parametrize("alpha", [0, 96, 255])
@pytest.mark.parametrize("n,h,w", [(3, 5, 7), (2, 9, 65), (2, 112, 112)])
def test_overlay_is_the_integer_blend(alpha, n, h, w):
    from glfusion_amd import data
    x, f = _logits(n, 5, h, w), _frames(n, h, w)
    want_l = V.labels_ref(x)
    grey = torch.from_numpy(V.grey_ref(f))
    if n * h * w >= 256:
        assert grey.flatten()[:256].tolist() == list(range(256))             # level / 255.0 comes back as level, every level
    labels, rgba = data.render_labels(x.to(DEV), frames=f.to(DEV), alpha=alpha)
    rgba = rgba.cpu()
    assert torch.equal(labels.cpu(), want_l)
    assert torch.equal(rgba, V.rgba_ref(want_l, data.PALETTE, f, alpha))
    assert bool((rgba[..., 3] == 255).all())
    bg = want_l == 0
    assert torch.equal(rgba[..., :3][bg].long(), grey[bg].unsqueeze(-1).expand(-1, 3))
    if alpha == 0:
        assert torch.equal(rgba[..., :3].long(), grey.unsqueeze(-1).expand(-1, -1, -1, 3))
    if alpha == 255:
        assert torch.equal(rgba[~bg], V.rgba_ref(want_l, data.PALETTE)[~bg])
    if h == 112:                                                             # the planted frame values: below 0, above 1, NaN
        assert [int(grey.flatten()[260 + 7 * k]) for k in range(3)] == [0, 255, 0]
    with pytest.raises(RuntimeError, match="alpha"):
        data.render_labels(x.to(DEV), frames=f.to(DEV), alpha=256)


@pytest.mark.parametrize("view", ["1", "2", "3", "4"])
def test_render_of_masks_is_the_ground_truth_formula(view):
    from glfusion_amd import data
    g = torch.Generator().manual_seed(int(view))
    lab = (torch.rand(97, 131, 3, generator=g) * 5).floor()
    _, masks = data.prepare_frames(None, lab.to(DEV), view)
    want = V.literal_labels(masks.cpu())                                     # main.py:610-612
    labels, rgba = data.render_labels(masks)
    assert torch.equal(labels.cpu().long(), want)
    assert torch.equal(rgba.cpu(), torch.tensor(data.PALETTE, dtype=torch.uint8)[want])
    shown = {ch + 1 for ch in data.CLASS_TO_CHANNEL[view] if ch >= 0}
    assert set(want.unique().tolist()) == shown | {0}


@pytest.mark.parametrize("view", ["1", "2", "3", "4"])
@pytest.mark.parametrize("h0,w0,t,offset", [(200, 160, 7, None), (600, 800, 3, (5, 31)), (97, 131, 1, (32, 0)), (144, 144, 4, (0, 32))])
def test_restore_labels_matches_restatement(view, h0, w0, t, offset):
    from glfusion_amd import data
    g = torch.Generator().manual_seed(h0 * 7 + t + int(view))
    x = V.plant(torch.randn(t, 5, 112, 112, generator=g) * 3)
    want = V.restore_ref(x, data.CHANNEL_TO_CLASS[view], (h0, w0), offset)
    got = data.restore_labels(x.to(DEV), view, (h0, w0, t), crop_offset=offset)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h0, w0, t) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    shown = {k + 1 for k, ch in enumerate(data.CLASS_TO_CHANNEL[view]) if ch >= 0}
    assert set(want.unique().tolist()) == shown | {0}
    outside = ~V.window_ref((h0, w0), crop_offset=offset)
    assert bool(outside.any()) and int(got.cpu()[outside].sum()) == 0


def test_restore_labels_many_frames():
    """More frames than one tile holds (64), not a multiple of it; a source narrower than one tile."""
    from glfusion_amd import data
    x = V.plant(torch.randn(70, 5, 112, 112, generator=torch.Generator().manual_seed(70)) * 3)
    want = V.restore_ref(x, data.CHANNEL_TO_CLASS["4"], (37, 50))
    assert torch.equal(data.restore_labels(x.to(DEV), "4", (37, 50)).cpu(), want)


@pytest.mark.parametrize("view", ["1", "2", "3", "4"])
def test_restore_round_trip(view):
    """At H0 = W0 = 144 the resize is the identity: restore_labels(prepare_frames(lab) * 20 - 10) gives lab back inside the crop
    window for the classes the view shows, 0 for those it does not, 0 outside the window."""
    from glfusion_amd import data
    lab = (torch.rand(144, 144, 4, generator=torch.Generator().manual_seed(40 + int(view))) * 5).floor()
    for offset in (None, (3, 29)):
        _, masks = data.prepare_frames(None, lab.to(DEV), view, crop_offset=offset)
        got = data.restore_labels(masks * 20 - 10, view, lab.shape, crop_offset=offset).cpu()
        oy, ox = (16, 16) if offset is None else offset
        n_parts = sum(ch >= 0 for ch in data.CLASS_TO_CHANNEL[view])
        want = torch.zeros(144, 144, 4)
        want[oy:oy + 112, ox:ox + 112] = lab[oy:oy + 112, ox:ox + 112]
        want[want > n_parts] = 0
        assert torch.equal(got, want.to(torch.uint8))
        assert int((want > 0).sum()) > 0 and bool((lab > n_parts).any()) == (n_parts < 4)


def test_restore_tie_break_and_unshown_channels():
    from glfusion_amd import data
    x = torch.full((2, 5, 112, 112), -5.0)
    x[1, 1, 0, 0] = x[1, 3, 0, 0] = 2.0                                     # a tie between shown channels: the lower channel's class
    x[1, 1, 0, 1], x[1, 3, 0, 1] = 2.0, 3.0                                  # unequal: the larger one's
    x[1, 1, 0, 2], x[1, 3, 0, 2] = 3.0, 2.0
    x[1, 4, 0, 3] = 9.0                                                      # view 1 does not show channel 4
    x[1, 4, 0, 4], x[1, 3, 0, 4] = 9.0, 0.5                                  # ... which does not outvote a shown channel either
    x[1, 0, 0, 5] = x[1, 2, 0, 5] = float("inf")
    vol = data.restore_labels(x.to(DEV), "1", (144, 144)).cpu()
    assert vol[16, 16:22, 1].tolist() == [2, 1, 2, 0, 1, 0] and int(vol.sum()) == 6
    assert torch.equal(vol, V.restore_ref(x, data.CHANNEL_TO_CLASS["1"], (144, 144)))
    with pytest.raises(RuntimeError, match="crop window"):
        data.restore_labels(x.to(DEV), "1", (144, 144), crop_offset=(40, 0))


def test_visual_mode_end_to_end(tmp_path):
    """Trainer.test_visualize on the fixture of test_eval_harness_vs_oracle: every file of the manifest, decoded, against the
    restatement on the very logits the pass rendered (the on_clip hook) and on oracle.prepare_clip's frames and masks."""
    from glfusion_amd import data, nifti
    from glfusion_amd.data import SyntheticPatients
    from glfusion_amd.engine import Trainer
    views = ["1", "4"]
    cfg = {"train": {"batch_size": 1, "num_epochs": 1, "clip_length": 3, "view_num": views, "test_view": views, "save_dir": str(tmp_path / "ckpt"),
                     "iters_per_epoch": 1, "global_rank": 0},
           "net": {"opt": {"opt_name": "Adam", "lr": 3e-4, "params": (0.9, 0.999), "weight_decay": 1e-5}}}
    t = Trainer(cfg)
    ref = orc.Global_and_Local(views)
    orc.closed_form_fill(ref, salt=9)
    t.model.load_state_dict(ref.state_dict(), strict=True)
    patients = SyntheticPatients(views, 2, clip_length=3, h0=150, w0=170, device=DEV, seed=5)
    seen = {}

    def on_clip(pid, view, logits, masks):
        assert logits.is_cuda and masks.is_cuda and (pid, view) not in seen
        seen[(pid, view)] = (logits.detach().cpu().clone(), masks.detach().cpu().clone())

    manifest = t.test_visualize("m", out_root=str(tmp_path), patients=patients, on_clip=on_clip)
    assert manifest is t.visual_report and sorted(manifest) == ["0_0", "0_1"] and sorted(seen) == [(p, v) for p in ("0_0", "0_1") for v in views]
    window = V.window_ref((150, 170))
    any_part = False
    for k, sample in enumerate(patients):
        pid = f"0_{k}"
        assert sorted(manifest[pid]) == views
        for v in views:
            entry = manifest[pid][v]
            png_dir = os.path.join(str(tmp_path), "m", "192_data", pid, v)
            nii = os.path.join(str(tmp_path), "m", "nifti", pid, f"view{v}_pred.nii.gz")
            assert entry == {"png_dir": png_dir, "nifti": nii, "frames": 3}
            assert sorted(os.listdir(png_dir)) == sorted(f"{kind}_{i}.png" for kind in ("pred", "gnd", "overlay") for i in range(3))
            logits, masks = seen[(pid, v)]
            frames, want_masks = orc.prepare_clip(sample[v][0].cpu(), sample[v][1].cpu(), v)
            assert tuple(logits.shape) == (3, 5, 112, 112) and torch.equal(masks, want_masks)
            pred_l, gnd_l = V.labels_ref(logits), V.labels_ref(want_masks)
            want = {"pred": V.rgba_ref(pred_l, data.PALETTE), "gnd": V.rgba_ref(gnd_l, data.PALETTE),
                    "overlay": V.rgba_ref(pred_l, data.PALETTE, frames, 96)}
            for kind, pictures in want.items():
                for i in range(3):
                    assert np.array_equal(V.decode_png(os.path.join(png_dir, f"{kind}_{i}.png")), pictures[i].numpy()), (pid, v, kind, i)
            vol = nifti.read(nii)
            assert vol.dtype == np.uint8 and vol.shape == (150, 170, 3)
            vol = torch.from_numpy(np.ascontiguousarray(vol))
            assert torch.equal(vol, V.restore_ref(logits, data.CHANNEL_TO_CLASS[v], (150, 170)))
            assert int(vol[~window].sum()) == 0
            any_part = any_part or int(gnd_l.max()) > 0
    assert any_part                                                           # the fixture is not degenerate
    # no overlay, no volumes, the backbone mask: only pred_ / gnd_ pictures, nothing under nifti/
    seen.clear()
    m2 = t.test_visualize("b", out_root=str(tmp_path), patients=patients, is_fuse=False, overlay_alpha=None, nifti=False, on_clip=on_clip)
    assert m2["0_1"]["4"]["nifti"] is None and not os.path.exists(os.path.join(str(tmp_path), "b", "nifti"))
    d = m2["0_1"]["4"]["png_dir"]
    assert sorted(os.listdir(d)) == sorted(f"{kind}_{i}.png" for kind in ("pred", "gnd") for i in range(3))
    assert np.array_equal(V.decode_png(os.path.join(d, "pred_2.png")), V.rgba_ref(V.labels_ref(seen[("0_1", "4")][0]), data.PALETTE)[2].numpy())
