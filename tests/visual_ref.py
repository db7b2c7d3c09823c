"""Helpers of tests/test_visual_cpu.py and tests/test_gpu_visual.py: the visual-mode kernels (csrc/data.hip: glf_render_labels,
glf_restore_labels) restated in numpy / torch CPU ops, a PNG decoder, and the planted logits.  A plain module, not a conftest.

Everything here is integer or index work, so every comparison against the kernels is torch.equal.  The one float decision is the
predicate sigmoid(logit) > 0.5, taken from oracle.binarize; the device evaluates 1 / (1 + expf(-x)) with its own expf, which can
differ from the host's in the last place, and only a logit in the open interval (0, 1e-6) sits near enough to the threshold
(sigmoid(x) - 0.5 ~ x / 4 against fp32 steps of 6e-8 there) for that to decide a pixel: `plant` keeps the inputs out of it.
"""
import struct
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle import glfusion_ref as orc

SPECIALS = (0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e-3, -1e-3)


def labels_ref(logits: torch.Tensor) -> torch.Tensor:
    """uint8 [N,H,W]: 0 when no channel is on, else 1 + the lowest channel that is on (= main.py:606-609, see literal_labels)."""
    on = orc.binarize(logits.float()) != 0                                   # [N,C,H,W]
    c = logits.shape[1]
    first = torch.where(on, torch.arange(1, c + 1).view(1, c, 1, 1), torch.full((), c + 1)).min(dim=1).values
    return torch.where(first > c, torch.zeros((), dtype=first.dtype), first).to(torch.uint8)


def literal_labels(x: torch.Tensor) -> torch.Tensor:
    """main.py:606-609 (and 610-612 for masks) word for word."""
    pred = torch.where(torch.sigmoid(x) > 0.5, 1, 0)
    return torch.argmax(torch.cat([0.5 + torch.zeros_like(pred[:, 0, :, :]).unsqueeze(1), pred], dim=1), dim=1)


def grey_ref(frames: torch.Tensor) -> np.ndarray:
    """int64 [N,H,W]: clamp((int)(v * 255.0f + 0.5f), 0, 255) with both operations rounded to fp32, NaN -> 0."""
    v = frames.reshape(frames.shape[0], frames.shape[-2], frames.shape[-1]).numpy().astype(np.float32)
    with np.errstate(invalid="ignore"):
        g = v * np.float32(255.0) + np.float32(0.5)
    g = np.where(np.isnan(g), np.float32(0.0), g)
    return np.clip(g, -1.0, 256.0).astype(np.int64).clip(0, 255)             # astype truncates toward zero, as (int) does


def rgba_ref(labels: torch.Tensor, palette, frames: torch.Tensor = None, alpha: int = 255) -> torch.Tensor:
    """uint8 [N,H,W,4]: palette[label]; with frames the integer blend over the grey level (grey where label == 0), opaque."""
    lab = labels.numpy().astype(np.int64)
    colour = np.asarray(palette, dtype=np.int64)[lab]                        # [N,H,W,4]
    if frames is not None:
        g = grey_ref(frames)[..., None]
        blend = (alpha * colour + (255 - alpha) * g + 127) // 255
        colour = np.where(lab[..., None] != 0, blend, np.broadcast_to(g, colour.shape)).copy()
        colour[..., 3] = 255
    return torch.from_numpy(colour.astype(np.uint8))


def restore_ref(logits: torch.Tensor, channel_to_class, shape, crop_offset=None, resize: int = 144) -> torch.Tensor:
    """uint8 [H0,W0,T]: per crop pixel the class of the channel with the largest logit among those that are on and mapped to a
    class (ties: the lowest channel -- torch.argmax returns the first maximum), 0 when none; that index image placed at the crop
    window of a zero resize x resize canvas and taken to H0 x W0 by F.interpolate(mode='nearest')."""
    t, c, oh, ow = logits.shape
    cls = torch.tensor(list(channel_to_class), dtype=torch.int64)
    valid = (orc.binarize(logits.float()) != 0) & (cls.view(1, c, 1, 1) != 0)
    best = torch.where(valid, logits.float(), torch.full((), float("-inf"))).argmax(dim=1)          # an on logit is > 0 > -inf
    idx = torch.where(valid.any(dim=1), cls[best], torch.zeros((), dtype=torch.int64))               # [T,oh,ow]
    oy, ox = ((resize - oh) // 2, (resize - ow) // 2) if crop_offset is None else crop_offset
    canvas = torch.zeros(t, 1, resize, resize)
    canvas[:, 0, oy:oy + oh, ox:ox + ow] = idx.float()
    vol = F.interpolate(canvas, size=(int(shape[0]), int(shape[1])), mode="nearest")[:, 0]           # [T,H0,W0]
    return vol.permute(1, 2, 0).contiguous().to(torch.uint8)


def window_ref(shape, oh: int = 112, ow: int = 112, crop_offset=None, resize: int = 144) -> torch.Tensor:
    """bool [H0,W0]: the source pixels whose nearest resized pixel lies inside the crop window."""
    ones = torch.ones(1, 1, oh, ow)
    return restore_ref(ones, (1,), shape, crop_offset, resize)[:, :, 0] != 0


def plant(logits: torch.Tensor) -> torch.Tensor:
    """In place: no logit in (0, 1e-6) (see the module docstring); where the tensor is large enough, an all-off pixel, a pixel with
    several channels on (all, when C > 1), and SPECIALS cycled over channels and pixels of the first image's first row(s)."""
    logits[(logits > 0) & (logits < 1e-6)] = 1e-3
    n, c, h, w = logits.shape
    flat = logits[0].reshape(c, h * w)                                       # a view: logits is contiguous
    hw = h * w
    if hw >= 2:
        flat[:, 0] = -2.0
        flat[:, 1] = 1.5
    for k, s in enumerate(SPECIALS):
        if 2 + k < hw:
            flat[:, 2 + k] = -3.0
            flat[k % c, 2 + k] = s
        if 2 + len(SPECIALS) + k < hw:                                       # the special below a channel that is on: it must not matter
            flat[:, 2 + len(SPECIALS) + k] = s
            flat[c - 1, 2 + len(SPECIALS) + k] = 2.0
    return logits


def decode_png(path) -> np.ndarray:
    """uint8 [H,W,4] of an 8-bit RGBA, non-interlaced PNG whose rows all use filter type 0; every chunk's CRC is checked."""
    raw = open(path, "rb").read()
    assert raw[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head, end = 8, b"", None, False
    while pos < len(raw):
        n, tag = struct.unpack(">I4s", raw[pos:pos + 8])
        body = raw[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", raw[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        head = struct.unpack(">IIBBBBB", body) if tag == b"IHDR" else head
        idat += body if tag == b"IDAT" else b""
        end = end or tag == b"IEND"
        pos += 12 + n
    w, h = head[:2]
    assert end and head[2:] == (8, 6, 0, 0, 0), head
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 4 * w)
    assert not rows[:, 0].any(), "filter type 0 only"
    return rows[:, 1:].reshape(h, w, 4).copy()
