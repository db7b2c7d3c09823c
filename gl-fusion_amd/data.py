"""GPU side of the reference's data path (datasets/loader.py:190-498).

The reference loads a NIfTI volume per (patient, view) with nibabel, runs a MONAI transform chain on the CPU
(AddChannel -> Resized(144, 144, 'nearest') -> RandSpatialCrop / CenterSpatialCrop(112, 112) -> EnsureType), turns the
label map into per-view part masks re-ordered into 5 class channels (loader.py:298-316, 358-414) and scales the image by
1/255 (loader.py:325-327).  Here the raw volume goes to the GPU once and ONE kernel (glf_prepare_frames) writes the model's
input layout directly: frames [T,1,112,112] and masks [T,5,112,112] -- the `[1,1,H,W,T] -> permute -> reshape(-1,1,H,W)`
of main.py:361-365 / 495-499 included.  NIfTI files themselves are not shipped with the reference (absolute paths on the
authors' machine); `SyntheticPatients` produces volumes with the same tensor contract.
(The RandFlipd objects of loader.py:468-474 are constructed but never put into the Compose: no flip is applied.)
Training does not go sample by sample: `VolumeStore` keeps the raw volumes on the device (uint8 where they arrive so), `BatchLoader` /
`ClipLoader` mirror the reference's per-view DataLoaders (main.py:139, 143-145, 185-218) over `SegPAHDataset.plan` /
`AlignedVideoSegPAHDataset.plan` and cut each batch with one glf_prepare_batch launch per view.
The way out is here too: `render_labels` (the label maps and colours of main.py:606-634) and `restore_labels` (predictions back in the
source volume's geometry, the inverse of `prepare_frames`), the two kernels of Trainer.test_visualize.
"""
from __future__ import annotations

import ctypes as C
from collections import OrderedDict
from typing import Dict, Iterator, List, NamedTuple, Optional, Sequence, Tuple

import torch

from ._lib import SRC_F32, SRC_U8, FrameSrc, check, lib
from .ops import _chk, _contig, _p, _stream

# class id (1..4) -> channel of the 5-channel mask, per view: loader.py:298-316 (which parts a view shows) composed with
# mask_to_allclass (loader.py:358-414)
CLASS_TO_CHANNEL: Dict[str, Tuple[int, int, int, int]] = {
    "1": (3, 1, -1, -1),        # parasternal long axis: LV -> 3, RV -> 1
    "2": (4, -1, -1, -1),       # pulmonary artery long axis: PA -> 4
    "3": (3, 1, -1, -1),        # LV short axis: LV -> 3, RV -> 1
    "4": (3, 2, 0, 1),          # apical four chamber: LV -> 3, LA -> 2, RA -> 0, RV -> 1
}
RESIZE, CROP = 144, 112         # loader.py:462-463
# the way back: class id (0 = this view does not show the channel) of each of the 5 mask channels, per view
CHANNEL_TO_CLASS: Dict[str, Tuple[int, ...]] = {
    v: tuple(table.index(ch) + 1 if ch in table else 0 for ch in range(5)) for v, table in CLASS_TO_CHANNEL.items()}
# colour of label 0 (background) and labels 1..5 (1 + class channel), r, g, b, a: main.py:623-634
PALETTE: Tuple[Tuple[int, int, int, int], ...] = (
    (0, 0, 0, 255), (55, 255, 254, 255), (27, 255, 46, 255), (45, 0, 251, 255), (251, 13, 15, 255), (223, 48, 236, 255))


def prepare_frames(images: Optional[torch.Tensor], labels: Optional[torch.Tensor], view: str, train: bool = False,
                   crop_offset: Optional[Tuple[int, int]] = None, labelled: bool = True):
    """images / labels: raw volumes [H0, W0, T] (or [H0, W0] for a single frame) on the GPU, float32.
    Returns (frames [T,1,112,112], masks [T,5,112,112]); either is None when its input is.
    Eval: centre crop (loader.py:489).  Train: a random crop window (loader.py:480) -- drawn here on the host unless
    `crop_offset` = (y, x) is given.  Unlabelled clips (is_unlab, loader.py:325) keep raw grey levels (no / 255)."""
    if view not in CLASS_TO_CHANNEL:
        raise KeyError(f"glfusion_amd.data: no part table for view {view!r} (loader.py:298-316 defines views 1-4)")
    ref = images if images is not None else labels
    if ref is None:
        raise RuntimeError("prepare_frames: nothing to prepare")
    if ref.dim() == 2:
        images = images.unsqueeze(-1) if images is not None else None
        labels = labels.unsqueeze(-1) if labels is not None else None
        ref = images if images is not None else labels
    h0, w0, t = ref.shape
    if crop_offset is None:
        if train:
            oy = int(torch.randint(0, RESIZE - CROP + 1, ()).item())
            ox = int(torch.randint(0, RESIZE - CROP + 1, ()).item())
        else:
            oy = ox = (RESIZE - CROP) // 2
    else:
        oy, ox = int(crop_offset[0]), int(crop_offset[1])
    dev = ref.device
    frames = masks = None
    if images is not None:
        images = _contig(_chk(images, "image volume"))
        frames = torch.empty(t, 1, CROP, CROP, dtype=torch.float32, device=dev)
    if labels is not None:
        labels = _contig(_chk(labels, "label volume"))
        if labels.shape != ref.shape:
            raise RuntimeError("prepare_frames: image and label volumes differ in shape")
        masks = torch.empty(t, 5, CROP, CROP, dtype=torch.float32, device=dev)
    table = (C.c_int * 4)(*CLASS_TO_CHANNEL[view])
    check(lib.glf_prepare_frames(_p(images), _p(labels), _p(frames), _p(masks), h0, w0, t, RESIZE, CROP, CROP, oy, ox, table,
                                 255.0 if labelled else 1.0, _stream()), "prepare_frames")
    return frames, masks


def part_overlap_counts(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """int64 [C, 4] = (tp, fp, fn, tn) of sigmoid(logits) > 0.5 against target per class channel of [N,C,H,W] tensors
    (the per-part metrics of main.py:537-543; their sum over C is main.py:519's whole-view count)."""
    logits, target = _contig(_chk(logits, "logits")), _contig(_chk(target, "target"))
    if logits.shape != target.shape or logits.dim() != 4:
        raise RuntimeError("part_overlap_counts: [N,C,H,W] logits and targets of one shape expected")
    n, c, h, w = logits.shape
    counts = torch.empty(c, 4, dtype=torch.int64, device=logits.device)
    check(lib.glf_overlap_counts_nchw(_p(logits), _p(target), _p(counts), n, c, h * w, _stream()), "overlap_counts_nchw")
    return counts


def _percentile(percentile) -> int:
    if int(percentile) != percentile or not 0 <= int(percentile) <= 100:
        raise ValueError(f"contour metrics: the percentile is an integer 0..100 (got {percentile!r})")
    return int(percentile)


def contour_stats(logits: torch.Tensor, target: torch.Tensor, percentile: int = 95) -> Tuple[torch.Tensor, torch.Tensor]:
    """What the contour metrics are made of, in one launch (glf_contour_distances; no reference counterpart): [N,C,H,W] logits and
    targets -> (stats int64 [N,C,2,4] = (count, max_d2, d2_lo, d2_hi), sums float64 [N,C,2]) per frame, class channel and direction
    (0: prediction -> target, 1: target -> prediction).  A mask's contour is its on pixels (sigmoid(logit) > 0.5, the predicate
    part_overlap_counts counts with; target != 0) with a 4-neighbour that is off or outside the image; d2 is a contour pixel's exact
    squared distance in pixels to the other contour, d2_lo / d2_hi the two order statistics that bracket the `percentile`, sums the
    sum of sqrt(d2), bitwise reproducible.  An empty contour on either side: both directions keep their count, -1 and 0.0 elsewhere."""
    logits, target = _contig(_chk(logits, "logits")), _contig(_chk(target, "target"))
    if logits.shape != target.shape or logits.dim() != 4:
        raise RuntimeError("contour_stats: [N,C,H,W] logits and targets of one shape expected")
    pct = _percentile(percentile)
    n, c, h, w = logits.shape
    stats = torch.empty(n, c, 2, 4, dtype=torch.int64, device=logits.device)
    sums = torch.empty(n, c, 2, dtype=torch.float64, device=logits.device)
    check(lib.glf_contour_distances(_p(logits), _p(target), _p(stats), _p(sums), n, c, h, w, pct, _stream()), "contour_distances")
    return stats, sums


def contour_metrics(stats: torch.Tensor, sums: torch.Tensor, percentile: int = 95) -> Dict[str, torch.Tensor]:
    """contour_stats' output -> [N,C] device tensors, without a host read: 'hd' = sqrt(max over directions of max_d2), 'hdp' = the
    larger of the two directed percentiles P = sqrt(d2_lo) + frac * (sqrt(d2_hi) - sqrt(d2_lo)), frac = ((percentile * (count - 1))
    % 100) / 100 (numpy's linear interpolation; percentile per direction, then the larger), 'assd' = (sums[0] + sums[1]) /
    (count[0] + count[1]), all float64 and unspecified where the pair is not scored; and the bool masks 'scored' (both contours
    non-empty), 'missed' (target only), 'spurious' (prediction only), 'absent' (neither): exactly one is true per pair."""
    pct = _percentile(percentile)
    if stats.dim() != 4 or tuple(stats.shape[2:]) != (2, 4) or stats.dtype != torch.int64 or sums.dtype != torch.float64 \
            or tuple(sums.shape) != tuple(stats.shape[:3]):
        raise RuntimeError("contour_metrics: stats int64 [N,C,2,4] and sums float64 [N,C,2] expected")
    count = stats[..., 0]
    has_pred, has_target = count[..., 0] > 0, count[..., 1] > 0
    root = stats[..., 1:].clamp(min=0).double().sqrt()                    # [N,C,2,3]: max, lo, hi
    frac = ((pct * (count - 1)) % 100).double() / 100.0
    p = root[..., 1] + frac * (root[..., 2] - root[..., 1])
    return {"hd": root[..., 0].amax(dim=-1), "hdp": p.amax(dim=-1), "assd": sums.sum(dim=-1) / count.sum(dim=-1).clamp(min=1).double(),
            "scored": has_pred & has_target, "missed": has_target & ~has_pred, "spurious": has_pred & ~has_target,
            "absent": ~has_pred & ~has_target}


class ContourAccumulator:
    """One view's contour sums over a pass: `total` [C,7] float64 on the device = (sum hd, sum hdp, sum assd, scored, missed, spurious,
    absent) per class channel, over the (frame, channel) pairs added so far.  Everything is additive: `add` takes a clip, `+=`
    another accumulator, one all_reduce of `total` combines ranks, and `report` (or `reports` for several views at once) is the
    one host read at the end of a pass."""
    KEYS = ("hd", "hd95", "assd", "scored", "missed", "spurious", "absent")

    def __init__(self, channels: int = 5, device=None, percentile: int = 95):
        self.percentile = _percentile(percentile)
        self.total = torch.zeros(channels, 7, dtype=torch.float64, device=device)

    def add(self, logits: torch.Tensor, target: torch.Tensor) -> "ContourAccumulator":
        m = contour_metrics(*contour_stats(logits, target, self.percentile), self.percentile)
        scored = m["scored"]
        zero = torch.zeros((), dtype=torch.float64, device=scored.device)
        cols = [torch.where(scored, m[k], zero).sum(dim=0) for k in ("hd", "hdp", "assd")]
        cols += [m[k].sum(dim=0).double() for k in ("scored", "missed", "spurious", "absent")]
        self.total += torch.stack(cols, dim=1)
        return self

    def __iadd__(self, other) -> "ContourAccumulator":
        """acc += (logits, target) adds a clip; acc += another accumulator adds what it holds."""
        if isinstance(other, ContourAccumulator):
            self.total += other.total
            return self
        logits, target = other
        return self.add(logits, target)

    @staticmethod
    def report_from_rows(rows: Sequence[Sequence[float]]) -> dict:
        """[C][7] host numbers -> {'hd', 'hd95', 'assd': per-part means over the scored pairs (None without any), 'scored', 'missed',
        'spurious', 'absent': per-part pair counts, 'mean': (hd, hd95, assd) over all scored pairs of all parts, or None}."""
        out = {key: [row[i] / row[3] if row[3] > 0 else None for row in rows] for i, key in enumerate(ContourAccumulator.KEYS[:3])}
        for i, key in enumerate(ContourAccumulator.KEYS[3:]):
            out[key] = [int(round(row[3 + i])) for row in rows]
        n = sum(row[3] for row in rows)
        out["mean"] = tuple(sum(row[i] for row in rows) / n for i in range(3)) if n > 0 else None
        return out

    def report(self) -> dict:
        return self.report_from_rows(self.total.tolist())

    @staticmethod
    def reports(accs: "Dict[str, ContourAccumulator]", reduce: bool = False) -> Dict[str, dict]:
        """{view: accumulator} -> {view: report} with ONE collective (if `reduce` and several ranks run) and ONE host read for all views."""
        views = list(accs)
        if not views:
            return {}
        stacked = torch.stack([accs[v].total for v in views])
        if reduce:
            import torch.distributed as dist
            if dist.is_initialized() and dist.get_world_size() > 1:
                dist.all_reduce(stacked)
        return {v: ContourAccumulator.report_from_rows(rows) for v, rows in zip(views, stacked.tolist())}


def render_labels(logits: torch.Tensor, frames: Optional[torch.Tensor] = None, alpha: int = 255, palette=PALETTE):
    """The pictures of main.py:606-634 in one kernel (glf_render_labels).  logits [N,C,H,W] (C = 1..8, float32: predictions are
    fp32 under every precision; a 0/1 mask renders to the reference's `visual_gnd`) -> (labels uint8 [N,H,W], rgba uint8
    [N,H,W,4]).  label = argmax over [0.5, on_0, .., on_{C-1}], first maximum: 0 = no channel on, else 1 + the lowest channel
    with sigmoid(logit) > 0.5 -- the predicate part_overlap_counts counts with.  rgba = palette[label] (C + 1 rows r, g, b, a).
    With `frames` [N,1,H,W] in [0,1] the colours are laid over the grey frame instead (not in the reference): integer alpha
    0..255, (alpha * colour + (255 - alpha) * grey + 127) // 255 where label != 0, the grey level elsewhere, opaque."""
    logits = _contig(_chk(logits, "logits"))
    if logits.dim() != 4:
        raise RuntimeError("render_labels: [N,C,H,W] logits expected")
    n, c, h, w = logits.shape
    pal = [int(x) for row in palette for x in row]
    if len(pal) != 4 * (c + 1) or any(len(row) != 4 for row in palette) or not all(0 <= x <= 255 for x in pal):
        raise ValueError(f"render_labels: the palette needs {c + 1} rows of 4 bytes (label 0 and one per channel)")
    if int(alpha) != alpha:
        raise ValueError("render_labels: alpha is an integer 0..255")
    if frames is not None:
        frames = _contig(_chk(frames, "frames"))
        if frames.numel() != n * h * w or tuple(frames.shape[-2:]) != (h, w):
            raise RuntimeError("render_labels: frames [N,1,H,W] must match the logits")
    labels = torch.empty(n, h, w, dtype=torch.uint8, device=logits.device)
    rgba = torch.empty(n, h, w, 4, dtype=torch.uint8, device=logits.device)
    check(lib.glf_render_labels(_p(logits), _p(frames), _p(labels), _p(rgba), n, c, h, w, (C.c_uint8 * len(pal))(*pal), int(alpha),
                                _stream()), "render_labels")
    return labels, rgba


def restore_labels(logits: torch.Tensor, view: str, shape: Sequence[int], crop_offset: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """The inverse geometry of prepare_frames (glf_restore_labels; no reference counterpart): logits [T,C,112,112] of `view`
    -> class-id volume uint8 [H0,W0,T] with (H0, W0) = shape[:2], the source volume's geometry and axis order, ready for
    nifti.write next to the file the clip came from.  A source pixel takes the class of its nearest pixel of the 144 x 144
    resized image (0 outside the crop window; `crop_offset` None = the centre crop): among the channels that are on and that
    the view shows (CHANNEL_TO_CLASS), the one with the largest logit, the lowest channel on a tie; 0 when there is none."""
    if view not in CHANNEL_TO_CLASS:
        raise KeyError(f"glfusion_amd.data: no part table for view {view!r} (loader.py:298-316 defines views 1-4)")
    logits = _contig(_chk(logits, "logits"))
    if logits.dim() != 4 or logits.shape[1] != len(CHANNEL_TO_CLASS[view]):
        raise RuntimeError(f"restore_labels: [T,{len(CHANNEL_TO_CLASS[view])},H,W] logits expected")
    t, c, oh, ow = logits.shape
    h0, w0 = int(shape[0]), int(shape[1])
    oy, ox = ((RESIZE - oh) // 2, (RESIZE - ow) // 2) if crop_offset is None else (int(crop_offset[0]), int(crop_offset[1]))
    volume = torch.empty(h0, w0, t, dtype=torch.uint8, device=logits.device)
    table = (C.c_int * c)(*CHANNEL_TO_CLASS[view])
    check(lib.glf_restore_labels(_p(logits), _p(volume), t, c, oh, ow, h0, w0, RESIZE, oy, ox, table, _stream()), "restore_labels")
    return volume


class SyntheticPatients:
    """Stand-in for Seg_PAHDataset's files: per patient and view a raw grey-level volume [H0, W0, T] in [0, 255] and a
    label volume with class ids 0..k (k parts of that view, loader.py:298-316), deterministic per (seed, patient, view).
    The parts are ellipses that drift over the frames, so Dice and the per-part tables are non-trivial."""

    PARTS = {"1": 2, "2": 1, "3": 2, "4": 4}

    def __init__(self, views: Sequence[str], n_patients: int, clip_length: int = 40, h0: int = 200, w0: int = 160, device="cuda", seed: int = 0):
        self.views, self.n, self.t, self.h0, self.w0, self.device, self.seed = list(views), n_patients, clip_length, h0, w0, device, seed

    def __len__(self) -> int:
        return self.n

    def volume(self, patient: int, view: str):
        g = torch.Generator().manual_seed(self.seed * 1000003 + patient * 101 + int(view))
        yy = torch.arange(self.h0, dtype=torch.float32).view(-1, 1, 1)
        xx = torch.arange(self.w0, dtype=torch.float32).view(1, -1, 1)
        tt = torch.arange(self.t, dtype=torch.float32).view(1, 1, -1)
        lab = torch.zeros(self.h0, self.w0, self.t)
        img = torch.rand(self.h0, self.w0, self.t, generator=g) * 60.0
        for k in range(1, self.PARTS[view] + 1):
            cy, cx = (torch.rand(2, generator=g) * 0.5 + 0.25).tolist()
            ry, rx = (torch.rand(2, generator=g) * 0.12 + 0.08).tolist()
            inside = (((yy - (cy + 0.02 * torch.sin(tt / 5.0)) * self.h0) / (ry * self.h0)) ** 2
                      + ((xx - (cx + 0.02 * torch.cos(tt / 7.0)) * self.w0) / (rx * self.w0)) ** 2) <= 1.0
            lab = torch.where(inside, torch.full_like(lab, float(k)), lab)
            img = torch.where(inside, img + 40.0 * k, img)
        return img.clamp_(0, 255).floor_().to(self.device), lab.to(self.device)

    def __iter__(self) -> Iterator:
        for p in range(self.n):
            yield {v: self.volume(p, v) for v in self.views}


# ------------------------------------------------------------------------------------------------------------
# host side of the loader: the Dataset contract of datasets/loader.py:190-340
# ------------------------------------------------------------------------------------------------------------
def crop_offsets(rs, size=(RESIZE, RESIZE), crop=(CROP, CROP)) -> Tuple[int, ...]:
    """Top-left corner of a RandSpatialCropd(roi_size=crop, random_size=False) window on an image of `size`, drawn from the
    numpy RandomState `rs` the way MONAI draws it (monai.data.utils.get_random_patch: one `rs.randint(low=0, high=ms - ps + 1)`
    per spatial dimension, in order, only where the image is larger than the patch) -- so a caller that seeds the transform's
    RandomState like the reference (loader.py:478-484; MONAI's Randomizable.set_random_state) gets the reference's windows.
    MONAI is not installed here: restated from its published source, parity unpinned."""
    return tuple(int(rs.randint(low=0, high=ms - ps + 1)) if ms > ps else 0 for ms, ps in zip(size, crop))


class SegPAHDataset:
    """Seg_PAHDataset (datasets/loader.py:190-340) with the file access factored out: `infos[id]` is a dict with
    'dataset_name', 'views_images' and 'views_labels', whose per-view entries are NIfTI-1 paths (what the reference stores
    there, loader.py:233-234; read by glfusion_amd.nifti), raw volumes [H0, W0, T] (numpy / torch) or zero-argument callables
    returning them.
    Everything else follows the reference: the train / val / test split of the id list (loader.py:210-217), 4 samples per
    patient and epoch in train mode (loader.py:289, 335-338), the labelled-frame selection `input_select` (loader.py:429-458:
    Python's `random` module, so `random.seed` reproduces the reference's picks), the transform chain and the part masks --
    the last two on the GPU in one kernel (prepare_frames).  Returns (images, masks, index) in the reference's layouts:
    images [1,112,112] or [1,112,112,T] scaled by 1/255, masks [5,112,112(,T)]."""

    def __init__(self, infos: dict, root=None, is_train: bool = True, data_list=None, set_select=("rmyy",), view_num=("2",),
                 single_frame: bool = True, clip_length: int = 32, seg_parts: bool = True, require_id: bool = False,
                 device="cuda", crop_seed=None, store: Optional["VolumeStore"] = None):
        import random
        import numpy as np
        if len(view_num) != 1:
            raise ValueError("SegPAHDataset: one view per dataset object, as in the reference (main.py:112-121 builds one per view)")
        self.is_train, self.view_num, self.single_frame = is_train, list(view_num), single_frame
        self.clip_length, self.seg_parts, self.require_id, self.device = clip_length, seg_parts, require_id, device
        self.store = store                                   # where plan() finds its volumes; __getitem__ never uses it
        self.data_dict = {k: v for k, v in infos.items() if v["dataset_name"] in set_select}          # get_dict, loader.py:416-427
        self.id_list = list(self.data_dict.keys())
        if data_list is not None:
            self.id_list = list(data_list)
        elif is_train:                                                                             # loader.py:213-217
            self.train_list = random.sample(self.id_list, int(len(self.id_list) * 0.8))
            rest = list(set(self.id_list).difference(set(self.train_list)))
            self.valid_list = random.sample(rest, int(len(rest) * 0.5))
            self.test_list = list(set(self.id_list).difference(set(self.train_list)).difference(set(self.valid_list)))
            self.id_list = self.train_list
        self.R = np.random.RandomState(crop_seed)            # the RandSpatialCropd's own RandomState (MONAI Randomizable)

    def __len__(self) -> int:
        return len(self.id_list) * 4 if self.is_train else len(self.id_list)

    @staticmethod
    def _volume(entry):
        import os
        import numpy as np
        if isinstance(entry, (str, os.PathLike)):                # the reference's case: a NIfTI path (loader.py:233-234)
            from . import nifti
            entry = nifti.read(entry)
        v = entry() if callable(entry) else entry
        return v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))

    def input_select(self, images: torch.Tensor, masks: torch.Tensor):
        """loader.py:429-458.  Frames whose label map holds more than 100 labelled pixels are candidates; one is drawn with
        random.choice; a clip of clip_length - 1 frames around it (start drawn with random.randint) in clip mode."""
        import random
        if masks.dim() >= 3:
            per_frame = masks.sum(dim=(0, 1))
            cand = torch.nonzero(per_frame > 100).flatten().tolist()
            if not cand:
                raise RuntimeError("SegPAHDataset: no labelled frame in this volume (the reference's random.choice raises here too)")
            index = random.choice(cand)
            if self.single_frame:
                return images[:, :, index], masks[..., index], index
            if masks.shape[-1] == 3:
                return images[:, :, 1:2].repeat(1, 1, self.clip_length), masks[:, :, 1:2].repeat(1, 1, self.clip_length), index
            r_index = random.randint(0, index if index < self.clip_length - 1 else self.clip_length - 1)
            start = index - r_index
            end = start + self.clip_length - 1
            return images[:, :, start:end], masks[..., start:end], r_index
        if self.single_frame:
            return images, masks, 0
        return images.unsqueeze(-1).repeat(1, 1, self.clip_length), masks.unsqueeze(-1).repeat(1, 1, self.clip_length), 0

    def __getitem__(self, index: int):
        view = self.view_num[0]
        pid = self.id_list[index // 4] if self.is_train else self.id_list[index]
        entry = self.data_dict[pid]
        img_e, lab_e = entry["views_images"].get(view), entry["views_labels"].get(view)
        if img_e is None or lab_e is None:                       # loader.py:262-279: a patient without this view -> zeros
            shape = (1, CROP, CROP) if self.single_frame else (1, CROP, CROP, self.clip_length)
            imgs = torch.zeros(shape, device=self.device)
            masks = torch.zeros((5,) + shape[1:], device=self.device)
            return (imgs, masks, 0, pid) if self.require_id else (imgs, masks, 0)
        images, labels = self._volume(img_e).float(), self._volume(lab_e).float()
        images, labels, idx = self.input_select(images, labels)
        offs = crop_offsets(self.R) if self.is_train else None
        frames, masks = prepare_frames(images.to(self.device), labels.to(self.device), view, train=self.is_train, crop_offset=offs)
        if not self.seg_parts:                                   # loader.py:321: any part -> one foreground channel
            masks = (masks.sum(dim=1, keepdim=True) > 0).float()
        if self.single_frame:
            imgs, masks = frames[0], masks[0]                    # [1,112,112], [5,112,112]
        else:
            imgs, masks = frames.permute(1, 2, 3, 0), masks.permute(1, 2, 3, 0)      # [1,112,112,T], [5,112,112,T] (views)
        return (imgs, masks, idx, pid) if self.require_id else (imgs, masks, idx)

    def _draw(self, sums: Optional[Sequence[int]]):
        """input_select's draws (loader.py:429-458) from the per-frame label sums alone, no pixel touched: the same calls to
        `random` in the same order.  sums None = a 2-D volume (no draw).  Returns (((t0, nt), ...), index)."""
        import random
        if sums is None:
            return ((0, 1),) * (1 if self.single_frame else self.clip_length), 0
        cand = [t for t, s in enumerate(sums) if s > 100]
        if not cand:
            raise RuntimeError("SegPAHDataset: no labelled frame in this volume (the reference's random.choice raises here too)")
        index = random.choice(cand)
        if self.single_frame:
            return ((index, 1),), index
        if len(sums) == 3:
            return ((1, 1),) * self.clip_length, index
        r_index = random.randint(0, index if index < self.clip_length - 1 else self.clip_length - 1)
        start = index - r_index
        return ((start, min(start + self.clip_length - 1, len(sums)) - start),), r_index      # a slice past the end comes back short

    def plan(self, index: int, store: Optional["VolumeStore"] = None) -> "FramePlan":
        """What __getitem__(index) would read, without reading it: the volumes (resident in `store`, default the dataset's), the
        frames and the crop window, after exactly __getitem__'s draws in its order -- random.choice over the labelled frames
        (from the store's cached sums), random.randint for the clip start, the crop window from the dataset's RandomState.
        prepare_batch turns any number of plans into one launch."""
        store = store if store is not None else self.store
        if store is None:
            raise RuntimeError("SegPAHDataset.plan needs a VolumeStore (the dataset's store= or the call's)")
        view = self.view_num[0]
        pid = self.id_list[index // 4] if self.is_train else self.id_list[index]
        entry = self.data_dict[pid]
        img_e, lab_e = entry["views_images"].get(view), entry["views_labels"].get(view)
        if img_e is None or lab_e is None:                       # loader.py:262-279: a patient without this view -> zeros
            return FramePlan(pid, view, None, None, ((0, 1 if self.single_frame else self.clip_length),), (0, 0), 0)
        lab = store.volume(pid, view, "label", lab_e)
        segments, idx = self._draw(store.frame_sums(pid, view, lab))
        off = crop_offsets(self.R) if self.is_train else ((RESIZE - CROP) // 2,) * 2
        img = store.volume(pid, view, "image", img_e)
        if img.shape != lab.shape:
            raise RuntimeError("SegPAHDataset: image and label volumes differ in shape")
        return FramePlan(pid, view, img, lab, segments, off, idx)


class FrameSource(NamedTuple):
    """One source of prepare_batch: frames t0 .. t0 + nt - 1 of a device volume pair [H0, W0, T] (or [H0, W0]), uint8 or float32
    each.  img None: nt frames of zeros.  lab None: no masks from this source.  view: the part table of the masks."""
    img: Optional[torch.Tensor]
    lab: Optional[torch.Tensor]
    t0: int = 0
    nt: int = 1
    view: Optional[str] = None
    off: Tuple[int, int] = ((RESIZE - CROP) // 2, (RESIZE - CROP) // 2)
    resize: int = RESIZE
    img_div: float = 255.0


class FramePlan(NamedTuple):
    """A dataset sample before any pixel is read: frames `segments` = ((t0, nt), ...) of the resident volumes, cropped at `off`;
    `index` is what the dataset returns as its third value."""
    pid: object
    view: str
    img: Optional[torch.Tensor]
    lab: Optional[torch.Tensor]
    segments: Tuple[Tuple[int, int], ...]
    off: Tuple[int, int]
    index: int
    resize: int = RESIZE
    img_div: float = 255.0

    def sources(self) -> List[FrameSource]:
        return [FrameSource(self.img, self.lab, t0, nt, self.view, self.off, self.resize, self.img_div) for t0, nt in self.segments]


def _device_volume(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.uint8, torch.float32) or t.dim() not in (2, 3):
        raise RuntimeError(f"glfusion_amd: {name} must be a CUDA(HIP) uint8 or float32 volume [H0, W0(, T)] (got "
                           f"{getattr(t, 'device', None)}, {getattr(t, 'dtype', None)}). The engine has no CPU fallback.")
    return _contig(t)


def prepare_batch(sources: Sequence[FrameSource], out_h: int = CROP, out_w: int = CROP, masks: bool = True, device=None):
    """glf_prepare_batch: the frames of all `sources`, in order, in ONE call -- (frames [sum nt, 1, out_h, out_w], masks
    [sum nt, 5, out_h, out_w] or None).  Per source the arithmetic is prepare_frames' (the kernels share the body), whatever
    the storage of its volumes.  `device`: where the outputs live when no source has a volume."""
    sources = list(sources)
    if not sources:
        raise RuntimeError("prepare_batch: no sources")
    descs = (FrameSrc * len(sources))()
    keep = []                                                    # contiguous copies must outlive the launch
    for d, s in zip(descs, sources):
        d.nt = int(s.nt)
        if s.img is None:
            continue
        img = _device_volume(s.img, "image volume")
        keep.append(img)
        device = img.device
        d.img, d.img_dtype = img.data_ptr(), SRC_U8 if img.dtype == torch.uint8 else SRC_F32
        d.H0, d.W0, d.T = img.shape[0], img.shape[1], img.shape[2] if img.dim() == 3 else 1
        d.t0, d.resize, d.off_y, d.off_x, d.img_div = int(s.t0), int(s.resize), int(s.off[0]), int(s.off[1]), float(s.img_div)
        if s.lab is not None and masks:
            lab = _device_volume(s.lab, "label volume")
            if lab.shape != img.shape:
                raise RuntimeError("prepare_batch: image and label volumes differ in shape")
            if s.view not in CLASS_TO_CHANNEL:
                raise KeyError(f"glfusion_amd.data: no part table for view {s.view!r} (loader.py:298-316 defines views 1-4)")
            keep.append(lab)
            d.lab, d.lab_dtype = lab.data_ptr(), SRC_U8 if lab.dtype == torch.uint8 else SRC_F32
            d.class_to_channel[:] = CLASS_TO_CHANNEL[s.view]
    if device is None or torch.device(device).type != "cuda":
        raise RuntimeError("prepare_batch: the outputs need a CUDA(HIP) device. The engine has no CPU fallback.")
    n = sum(int(s.nt) for s in sources)
    with torch.cuda.device(device):
        frames = torch.empty(n, 1, out_h, out_w, dtype=torch.float32, device=device)
        out_masks = torch.empty(n, 5, out_h, out_w, dtype=torch.float32, device=device) if masks else None
        check(lib.glf_prepare_batch(descs, len(sources), _p(frames), _p(out_masks), out_h, out_w, _stream()), "prepare_batch")
    return frames, out_masks


def frame_label_sums(labels: torch.Tensor) -> torch.Tensor:
    """glf_frame_label_sums: int64 [T] = labels.sum(dim=(0, 1)) of a device class-id volume [H0, W0, T], uint8 or float32."""
    labels = _device_volume(labels, "label volume")
    if labels.dim() != 3:
        raise RuntimeError("frame_label_sums: a [H0, W0, T] volume expected")
    h0, w0, t = labels.shape
    with torch.cuda.device(labels.device):
        sums = torch.empty(t, dtype=torch.int64, device=labels.device)
        check(lib.glf_frame_label_sums(_p(labels), SRC_U8 if labels.dtype == torch.uint8 else SRC_F32, h0, w0, t, _p(sums), _stream()),
              "frame_label_sums")
    return sums


class VolumeStore:
    """Raw volumes resident on the device, keyed by (patient id, view, 'image' | 'label' | 'video'), least recently used out first within
    `max_bytes`.  A volume that arrives as uint8 (echo frames and label maps normally do) stays uint8, a quarter of the memory;
    anything else is stored as float32 -- the kernels read both and give the same bits.  A volume larger than the whole budget is
    served and not kept.  The per-frame sums of a label volume (what input_select compares with 100) are computed once on the
    device and kept on the host, beyond the volume's own stay."""

    def __init__(self, device="cuda", max_bytes: int = 8 << 30):
        self.device, self.max_bytes = torch.device(device), int(max_bytes)
        self._volumes: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()
        self._sums: Dict[tuple, Optional[Tuple[int, ...]]] = {}
        self.bytes = 0                                           # of the volumes held now
        self.loads = 0                                           # volumes read and uploaded so far

    def __len__(self) -> int:
        return len(self._volumes)

    def volume(self, pid, view: str, kind: str, entry) -> torch.Tensor:
        """The device volume of `entry` (what SegPAHDataset._volume accepts: a NIfTI path, an array, a callable)."""
        key = (pid, view, kind)
        v = self._volumes.get(key)
        if v is not None:
            self._volumes.move_to_end(key)
            return v
        v = SegPAHDataset._volume(entry)
        v = _contig((v if v.dtype == torch.uint8 else v.float()).to(self.device))
        self.loads += 1
        size = v.numel() * v.element_size()
        while self._volumes and self.bytes + size > self.max_bytes:
            _, old = self._volumes.popitem(last=False)
            self.bytes -= old.numel() * old.element_size()
        if size <= self.max_bytes:
            self._volumes[key] = v
            self.bytes += size
        return v

    def frame_sums(self, pid, view: str, labels: torch.Tensor) -> Optional[Tuple[int, ...]]:
        """Host tuple of the per-frame sums of the (pid, view) label volume `labels` (the store's own tensor); None for a 2-D one."""
        key = (pid, view)
        if key not in self._sums:
            self._sums[key] = tuple(frame_label_sums(labels).tolist()) if labels.dim() == 3 else None
        return self._sums[key]


class AlignedVideoSegPAHDataset:
    """Aligned_Video_Seg_PAHDataset (datasets/loader.py:964-1069), the unlabelled clips of the cycle term: the same `infos` and
    id split as SegPAHDataset, one sample per patient.  The window rule of loader.py:1008-1019 on the frame axis: more frames
    than clip_length -> the first clip_length (random_sample: clip_length from random.randint(0, T - clip_length - 1)); fewer
    -> the volume followed by itself once; equal -> unchanged.  A trailing singleton axis is squeezed.  A patient without
    the view is replaced by random.choice over the ids until one has it (loader.py:1025-1026).  Images are raw -- no resize,
    no crop, no / 255 -- [1, H, W, T'], masks the raw label volume [H, W, T'] as float; the index is 0 (loader.py:1007)."""

    def __init__(self, infos: dict, root=None, is_train: bool = True, data_list=None, set_select=("rmyy",), view_num=("2",),
                 clip_length: int = 32, require_id: bool = False, random_sample: bool = False):
        import random
        if len(view_num) != 1:
            raise ValueError("AlignedVideoSegPAHDataset: one view per dataset object, as in the reference (main.py:119-122)")
        self.is_train, self.view_num, self.clip_length = is_train, list(view_num), clip_length
        self.require_id, self.random_sample = require_id, random_sample
        self.data_dict = {k: v for k, v in infos.items() if v["dataset_name"] in set_select}          # get_dict, loader.py:1059-1069
        self.id_list = list(self.data_dict.keys())
        if data_list is not None:
            self.id_list = list(data_list)
        elif is_train:                                                                             # loader.py:985-991
            self.train_list = random.sample(self.id_list, int(len(self.id_list) * 0.8))
            rest = list(set(self.id_list).difference(set(self.train_list)))
            self.valid_list = random.sample(rest, int(len(rest) * 0.5))
            self.test_list = list(set(self.id_list).difference(set(self.train_list)).difference(set(self.valid_list)))
            self.id_list = self.train_list

    def __len__(self) -> int:
        return len(self.id_list)

    def window(self, t: int) -> Tuple[Tuple[int, int], ...]:
        """((t0, nt), ...) of a volume of t frames, loader.py:1008-1019; the one draw of random_sample is made here."""
        import random
        if t > self.clip_length:
            start = random.randint(0, t - self.clip_length - 1) if self.random_sample else 0
            return ((start, self.clip_length),)
        return ((0, t), (0, t)) if t < self.clip_length else ((0, t),)

    def _entries(self, pid):
        view, entry = self.view_num[0], self.data_dict[pid]
        img_e, lab_e = entry["views_images"].get(view), entry["views_labels"].get(view)
        return (img_e, lab_e) if img_e is not None and lab_e is not None else None

    def pick(self, index: int):
        """(patient id whose volumes are served, its entries): id_list[index], or random.choice draws until a patient has the view."""
        import random
        pid = self.id_list[index]
        if not any(self._entries(p) for p in self.id_list):
            raise RuntimeError(f"AlignedVideoSegPAHDataset: no patient of the list has view {self.view_num[0]} (the reference loops forever here)")
        while self._entries(pid) is None:
            pid = random.choice(self.id_list)
        return pid, self._entries(pid)

    @staticmethod
    def _squeezed(v: torch.Tensor) -> torch.Tensor:
        return v.squeeze(-1) if v.dim() == 4 and v.shape[-1] == 1 else v

    def __getitem__(self, index: int):
        _, (img_e, lab_e) = self.pick(index)
        images, labels = self._squeezed(SegPAHDataset._volume(img_e)), self._squeezed(SegPAHDataset._volume(lab_e))
        segments = self.window(images.shape[-1])
        images = torch.cat([images[..., t0:t0 + nt] for t0, nt in segments], dim=-1).unsqueeze(0)
        labels = torch.cat([labels[..., t0:t0 + nt] for t0, nt in segments], dim=-1).float()
        return (images, labels, 0, self.id_list[index]) if self.require_id else (images, labels, 0)

    def plan(self, index: int, store: "VolumeStore") -> FramePlan:
        """__getitem__'s draws, and the image volume resident in `store`, as the identity geometry of prepare_batch."""
        pid, (img_e, _) = self.pick(index)
        key = (pid, self.view_num[0], "video")          # not "image": the labelled-frame infos use the same patient ids
        img = store.volume(*key, lambda: self._squeezed(SegPAHDataset._volume(img_e)))
        if img.dim() != 3 or img.shape[0] != img.shape[1]:
            raise ValueError(f"AlignedVideoSegPAHDataset: clips are served unresized and the device path takes square frames; "
                             f"volume {key[:2]} is {tuple(img.shape)}")
        return FramePlan(pid, self.view_num[0], img, None, self.window(img.shape[-1]), (0, 0), 0, resize=img.shape[0], img_div=1.0)


class BatchLoader:
    """The reference's training loaders -- one DataLoader(batch_size=B, shuffle=False, drop_last=True) per view (main.py:139)
    stepped together (main.py:185-205) -- over per-view SegPAHDatasets whose volumes are resident in `store`.  len = len(first
    view's dataset) // B; iteration k takes the consecutive samples k B .. k B + B - 1 of every view; within an iteration the
    views come in the datasets' order and the samples in index order, so the random draws come in the order the reference's
    num_workers = 0 loaders make them.  One glf_prepare_batch call per view and iteration.  Yields (imgs, masks) dicts of
    [B * frames, 1, 112, 112] / [B * frames, 5, 112, 112], SyntheticClips.batch()'s contract; `indices` holds the frame
    indices of the last batch per view.  world > 1: rank r takes iterations r, r + world, ...; the remainder is dropped."""

    def __init__(self, datasets_by_view: Dict[str, SegPAHDataset], batch_size: int, store: VolumeStore, rank: int = 0, world: int = 1):
        if batch_size < 1 or world < 1 or not 0 <= rank < world or not datasets_by_view:
            raise ValueError("BatchLoader: batch_size >= 1, 0 <= rank < world and at least one view expected")
        self.datasets, self.batch_size, self.store, self.rank, self.world = dict(datasets_by_view), batch_size, store, rank, world
        self.indices: Dict[str, List[int]] = {}

    def index_plan(self) -> List[List[int]]:
        """The sample indices of this rank's iterations of one epoch.  Host only."""
        b = self.batch_size
        iterations = len(next(iter(self.datasets.values()))) // b
        iterations -= iterations % self.world
        return [list(range(k * b, (k + 1) * b)) for k in range(self.rank, iterations, self.world)]

    def __len__(self) -> int:
        return len(self.index_plan())

    def __iter__(self) -> Iterator:
        for idxs in self.index_plan():
            imgs, masks, self.indices = {}, {}, {}
            for view, ds in self.datasets.items():
                plans = [ds.plan(i, self.store) for i in idxs]
                imgs[view], masks[view] = prepare_batch([s for p in plans for s in p.sources()], device=self.store.device)
                if not ds.seg_parts:                             # loader.py:321: any part -> one foreground channel
                    masks[view] = (masks[view].sum(dim=1, keepdim=True) > 0).float()
                self.indices[view] = [p.index for p in plans]
            yield imgs, masks


class ClipLoader:
    """The reference's clip loaders (DataLoader(batch_size=1, shuffle=False, drop_last=True) per view, main.py:143-145) over
    per-view AlignedVideoSegPAHDatasets: yields {view: [T', 1, H, W]} raw grey levels, the tensor main.py:216-218 reshapes to.
    world > 1: rank r takes clips r, r + world, ...  `batch()` is the engine's way in -- (clips, None), the next clip on each
    call; after the last clip it starts over (the reference's iterator would end there, main.py:215)."""

    def __init__(self, datasets_by_view: Dict[str, AlignedVideoSegPAHDataset], store: VolumeStore, rank: int = 0, world: int = 1):
        if world < 1 or not 0 <= rank < world or not datasets_by_view:
            raise ValueError("ClipLoader: 0 <= rank < world and at least one view expected")
        self.datasets, self.store, self.rank, self.world = dict(datasets_by_view), store, rank, world
        self._cursor = None

    def __len__(self) -> int:
        return len(next(iter(self.datasets.values()))) // self.world

    def _clip(self, index: int) -> Dict[str, torch.Tensor]:
        clips = {}
        for view, ds in self.datasets.items():
            plan = ds.plan(index, self.store)
            clips[view] = prepare_batch(plan.sources(), out_h=plan.resize, out_w=plan.resize, masks=False)[0]
        return clips

    def __iter__(self) -> Iterator:
        for k in range(len(self)):
            yield self._clip(self.rank + k * self.world)

    def batch(self):
        if len(self) == 0:
            raise RuntimeError("ClipLoader: no clips for this rank")
        try:
            if self._cursor is None:
                self._cursor = iter(self)
            return next(self._cursor), None
        except StopIteration:
            self._cursor = iter(self)
            return next(self._cursor), None


def load_infos(infos):
    """An `infos` dict as it is, or the reference's pickled .npy of one (np.load(...).item(), main.py:283)."""
    import os
    if isinstance(infos, (str, os.PathLike)):
        import numpy as np
        infos = np.load(infos, allow_pickle=True).item()
    if not isinstance(infos, dict):
        raise TypeError("glfusion_amd.data: infos is a dict {id: {'dataset_name', 'fold', 'views_images', 'views_labels'}} or a path to its .npy")
    return infos


def synthetic_infos(views: Sequence[str], n_patients: int, clip_length: int = 40, device="cpu", seed: int = 0, fold: str = "0",
                    h0: int = 200, w0: int = 160) -> dict:
    """An `infos` dict in the reference's shape (np.load('./infos/...npy') of main.py:283) whose volume entries are lazy
    SyntheticPatients volumes: ids '<fold>_<k>' like the reference's ('0_0', '0_2' = validation, the rest = test, main.py:288-289)."""
    sp = SyntheticPatients(views, n_patients, clip_length, h0=h0, w0=w0, device=device, seed=seed)
    infos = {}
    for k in range(n_patients):
        infos[f"{fold}_{k}"] = {"dataset_name": "rmyy", "fold": fold,
                                "views_images": {v: (lambda k=k, v=v: sp.volume(k, v)[0]) for v in views},
                                "views_labels": {v: (lambda k=k, v=v: sp.volume(k, v)[1]) for v in views}}
    return infos
